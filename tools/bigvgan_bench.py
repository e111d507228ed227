"""dev: time of the BigVGAN vocoder (audio.BigVGAN: gt_voc_snake in front of gt_voc_conv) against the same generator and
weights as plain PyTorch-ROCm conv1d / conv_transpose1d on the same device.

Two shapes, the published base shape with random weights and log alpha / beta uniform in [-1, 1]: the bench batch (B = 32 utterances of
800 frames) and ONE 800-frame utterance.  Per shape:
  kernel      BigVGAN.run (78 gt_voc_conv + 73 gt_voc_snake launches) captured in one graph and replayed; device events around
              >= --seconds of replays with a synchronise behind them, --repeats windows, the best and every window recorded.  The
              single utterance rotates over three workspaces and mels (one workspace alone would sit in the 256 MB Infinity Cache).
  stages      the same launches cut into conv_pre, the four upsampling stages (transposed convolution + three AMP blocks) and the end
              (activation_post + conv_post), one graph each; and per stage the activation launches ALONE (the convolutions skipped: they
              read what the last full run left in the buffers, values of the real magnitudes), with the bytes an ideal launch moves
              (4 in, 2 out per element) and their share of the 6.29 TB/s measured HBM copy rate in the measured time.
  torch       eager F.conv1d / F.conv_transpose1d (the published Activation1d: replicate padding, grouped transposed convolution, snake,
              replicate padding, grouped strided convolution) on the padded batch (all utterances have one length, so the padded batch
              IS the per-utterance definition), fp32 and under bf16 autocast, alternating with the kernel in every repeat.
Outputs are compared once per shape: relative L2 of the kernel path and of the bf16 torch path against the fp32 torch result.
The kernel phases of BOTH shapes run first and are written before any torch formulation starts (its first calls search for algorithms).

    python tools/bigvgan_bench.py [--json profiles/bigvgan_bench.json] [--seconds 0.5] [--repeats 3] [--shapes a,b] [--no-torch]"""
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
ap.add_argument("--json", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bigvgan_bench.json"))
ap.add_argument("--seconds", type=float, default=0.5)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--shapes", default="single_1x800,batch_32x800")
ap.add_argument("--no-torch", action="store_true", help="skip the PyTorch formulations (their first calls search for algorithms)")
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("bigvgan_bench needs the MI355X: there is nothing to time on a CPU")
dev = torch.device("cuda:0")
FRAMES, HBM, HIFIGAN_V1_MS = 800, 6.29e12, 45.6        # HiFi-GAN V1 on the bench batch: profiles/hifigan_bench.json
torch.manual_seed(0)
voc = audio.BigVGAN()
with torch.no_grad():
    for n_, p_ in voc.named_parameters():
        if n_.endswith(".alpha") or n_.endswith(".beta"):
            p_.uniform_(-1.0, 1.0)
voc = voc.to(dev)
K = len(voc.resblock_kernel_sizes)


def activation1d(x, act):
    C = x.shape[1]
    al, be = act.act.alpha.exp()[None, :, None], act.act.beta.exp()[None, :, None]
    fu, fd = act.upsample.filter.to(x.dtype).expand(C, -1, -1), act.downsample.lowpass.filter.to(x.dtype).expand(C, -1, -1)
    u = 2 * F.conv_transpose1d(F.pad(x, (5, 5), mode="replicate"), fu, stride=2, groups=C)[..., 15:-15]
    v = u + (1.0 / (be + 1e-9)) * torch.sin(u * al) ** 2
    return F.conv1d(F.pad(v, (5, 6), mode="replicate"), fd, stride=2, groups=C)


def torch_generator(mel):
    """the published generator on the module's own fp32 parameters"""
    x = F.conv1d(mel, voc.conv_pre.weight, voc.conv_pre.bias, padding=3)
    for i, ups in enumerate(voc.ups):
        up = ups[0]
        x = F.conv_transpose1d(x, up.weight, up.bias, stride=up.stride[0], padding=up.padding[0])
        xs = None
        for j in range(K):
            rb, y = voc.resblocks[i * K + j], x
            for m, (c1, c2) in enumerate(zip(rb.convs1, rb.convs2)):
                t = F.conv1d(activation1d(y, rb.activations[2 * m]), c1.weight, c1.bias, padding=c1.padding[0], dilation=c1.dilation[0])
                y = F.conv1d(activation1d(t, rb.activations[2 * m + 1]), c2.weight, c2.bias, padding=c2.padding[0]) + y
            xs = y if xs is None else xs + y
        x = xs / K
    return torch.tanh(F.conv1d(activation1d(x, voc.activation_post), voc.conv_post.weight, voc.conv_post.bias, padding=3))[:, 0]


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


PER_STAGE = (voc.launches - 3) // len(voc.ups)
STAGES = [("conv_pre", 0, 1)] + [(f"stage{i}", 1 + i * PER_STAGE, 1 + (i + 1) * PER_STAGE) for i in range(len(voc.ups))] + \
         [("end", voc.launches - 2, voc.launches)]


class Only:
    """BigVGAN's launches restricted to calls [lo, hi) of a run (snake_only: the activations among them), counting what they move"""

    def __init__(self, lo, hi, snake_only=False):
        self.lo, self.hi, self.snake_only, self.i, self.conv_bytes, self.snake_bytes, self.n = lo, hi, snake_only, 0, 0.0, 0.0, 0
        self.conv, self.snake = audio.BigVGAN._launch, audio.BigVGAN._snake

    def on_conv(self, m, dev_, n_frames, B, L, mul, X, img, Y, Cin, N, taps, dil, slope, x_sb, y_sb, ldy, **kw):
        if self.lo <= self.i < self.hi and not self.snake_only:
            self.conv_bytes += B * L * (Cin * (2 if kw.get("x_bf16") else 4) + N * 4
                                        + 4 * N * ((kw.get("res") is not None) + (kw.get("acc") is not None))) + img[0].numel() * 2
            self.n += 1
            self.conv(m, dev_, n_frames, B, L, mul, X, img, Y, Cin, N, taps, dil, slope, x_sb, y_sb, ldy, **kw)
        self.i += 1

    def on_snake(self, m, dev_, n_frames, B, L, mul, X, P, Y, C):
        if self.lo <= self.i < self.hi:
            self.snake_bytes += 6.0 * B * L * C
            self.n += 1
            self.snake(m, dev_, n_frames, B, L, mul, X, P, Y, C)
        self.i += 1

    def __enter__(self):
        audio.BigVGAN._launch = lambda m, *a, **k: self.on_conv(m, *a, **k)
        audio.BigVGAN._snake = lambda m, *a, **k: self.on_snake(m, *a, **k)
        return self

    def __exit__(self, *exc):
        audio.BigVGAN._launch, audio.BigVGAN._snake = self.conv, self.snake


T0 = time.time()
result = {"device": torch.cuda.get_device_name(0), "frames_per_utterance": FRAMES, "launches": voc.launches,
          "conv_launches": voc.conv_launches, "snake_launches": voc.snake_launches,
          "snake_tile_positions": audio.call.gt_voc_snake_tile_positions(), "hbm_bytes_per_s": HBM,
          "hifigan_v1_batch_ms": HIFIGAN_V1_MS, "shapes": {}}
state = {}


def write():
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:                                                   # after every phase: a later failure keeps the earlier one
        json.dump(result, f, indent=1)


def measure(times, variants):
    for _ in range(args.repeats):                                                     # the variants alternate inside every repeat
        for k, (fn, per_call) in variants.items():
            times.setdefault(k, []).append(window(fn, per_call))
            say(k, f"{times[k][-1]:.3f} ms")


def record(name, check):
    st = state[name]
    B, times, asked = st["B"], st["times"], st["asked"]
    best = {k: min(v) for k, v in times.items()}
    stages = {}
    for sname, _, _ in STAGES:
        conv_b, snake_b, n_snake = asked[sname]
        stages[sname] = {"ms": best[sname], "mbytes_conv": conv_b * 1e-6, "mbytes_snake": snake_b * 1e-6,
                         "share_of_hbm_rate": (conv_b + snake_b) / HBM * 1e3 / best[sname]}
        if n_snake:
            s_ms = best[sname + "_snake"]
            stages[sname].update({"snake_launches": n_snake, "snake_ms": s_ms, "snake_share_of_stage": s_ms / best[sname],
                                  "snake_tbytes_per_s": snake_b / s_ms * 1e-9, "snake_share_of_hbm_rate": snake_b / HBM * 1e3 / s_ms})
    snake_ms = sum(v.get("snake_ms", 0.0) for v in stages.values())
    snake_b = sum(v[1] for v in asked.values())
    shape = {"B": B, "audio_seconds_at_22050": B * FRAMES * 256 / 22050.0, "ms_best": best, "ms_windows": times, "outputs": check,
             "stages": stages, "stage_sum_share_of_kernel": sum(best[s] for s, _, _ in STAGES) / best["kernel"],
             "snake_ms_alone": snake_ms, "snake_share_of_kernel": snake_ms / best["kernel"],
             "snake_share_of_hbm_rate": snake_b / HBM * 1e3 / snake_ms,
             "real_time_factor": B * FRAMES * 256 / 22050.0 / (best["kernel"] * 1e-3)}
    if B == 32:
        shape["over_hifigan_v1"] = best["kernel"] / HIFIGAN_V1_MS
    for k in ("torch_fp32", "torch_bf16_autocast"):
        shape[k + "_over_kernel"] = best[k] / best["kernel"] if k in best else "not measured"
    result["shapes"][name] = shape
    write()
    return shape


SHAPES = [s for s in (("single_1x800", 1, 3), ("batch_32x800", 32, 1)) if s[0] in args.shapes.split(",")]
side = torch.cuda.Stream()
for name, B, rot in SHAPES:
    g = torch.Generator().manual_seed(B)
    mels = [(torch.rand(B, 80, FRAMES, generator=g) * 13.0 - 11.5).to(dev) for _ in range(rot)]
    n_frames = torch.full((B,), FRAMES, dtype=torch.int32, device=dev)
    works = [voc.workspace(B, FRAMES, dev) for _ in range(rot)]
    say(name, f"inputs ready, workspace {voc.workspace_bytes(B, FRAMES) / 1e9:.3f} GB x {rot}")
    for m, w in zip(mels, works):
        voc.run(m, n_frames, w)
    out_k = works[0]["wav"].clone()
    torch.cuda.synchronize()
    say("kernel path ran once")
    g_all = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g_all, stream=side):
        for m, w in zip(mels, works):
            voc.run(m, n_frames, w)
    graphs, asked = {"kernel": g_all}, {}
    for sname, lo, hi in STAGES:
        for snake_only in (False, True) if sname != "conv_pre" else (False,):
            gr = torch.cuda.CUDAGraph()
            with Only(lo, hi, snake_only) as only, torch.cuda.graph(gr, stream=side):
                for m, w in zip(mels, works):
                    only.i = 0
                    voc.run(m, n_frames, w)
            if snake_only and only.n:
                graphs[sname + "_snake"] = gr
            elif not snake_only:
                graphs[sname] = gr
                asked[sname] = [only.conv_bytes / rot, only.snake_bytes / rot, 0]
            if snake_only:
                asked[sname][2] = only.n // rot
    state[name] = dict(B=B, rot=rot, mels=mels, works=works, graphs=graphs, asked=asked, times={}, out_k=out_k)
    g_all.replay()                                                                    # the buffers hold a full run's values
    torch.cuda.synchronize()
    measure(state[name]["times"], {k: (gr.replay, rot) for k, gr in graphs.items()})
    g_all.replay()
    print(name, json.dumps(record(name, {})), flush=True)

if not args.no_torch:
    for name, B, rot in SHAPES:
        st = state[name]
        mels, g_all = st["mels"], st["graphs"]["kernel"]
        with torch.no_grad():
            out_t = torch_generator(mels[0])
            torch.cuda.synchronize()
            say(name, "torch fp32 ran once")
            out_b = torch_bf16(mels[0])
            torch.cuda.synchronize()
            say(name, "torch bf16 autocast ran once")
        nrm = torch.linalg.norm(out_t)
        check = {"kernel_vs_torch_fp32_rel_l2": (torch.linalg.norm(st["out_k"] - out_t) / nrm).item(),
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
        measure(st["times"], {"kernel": (g_all.replay, rot), "torch_fp32": (t32, 1), "torch_bf16_autocast": (t16, 1)})
        print(name, json.dumps(record(name, check)), flush=True)
print("wrote", args.json)
