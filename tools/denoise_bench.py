"""dev: time of the spectral-subtraction denoiser (audio.Denoiser on csrc/denoise.hip and gt_istft) against the
reference's formulation in PyTorch-ROCm on the same device and the same inputs, and what the stage costs behind WaveGlow.

Two shapes: the bench batch (B = 32 utterances of 800 mel frames = 204 800 samples each) and one 800-frame utterance.  Per shape:
  stage     Denoiser.run's two launches captured in graphs and replayed — gt_denoise_spec alone, gt_istft alone and the pair (10 calls
            per replay each); device events around >= --seconds of replays with a synchronise behind them, --repeats windows, the best
            and every window recorded.  Bytes: the analysis reads the samples (1 KB per frame) and writes the spectrum (8.2 KB per
            frame); `spec_gbps` is that over the kernel's time.
  torch     NVIDIA's Denoiser.forward, eager: F.pad(reflect) -> F.conv1d(forward_basis, stride 256) -> sqrt / atan2 ->
            clamp(mag - strength bias) -> cos / sin -> the inverse.  The inverse's transposed convolution is written as matmul + four
            shifted adds (the GEMM and the overlap-add it is) with the float32 squared-window envelope, as tools/gl_bench.py writes it
            and for its reason (F.conv_transpose1d with this filter did not return within minutes).  Same windows,
            alternating with the kernels.  The two outputs are compared sample by sample once per shape.
  waveglow  audio.WaveGlow at the published configuration with random weights (tools/waveglow_bench.py's initialisation): the graph of
            WaveGlow.run against the graph of Denoised(WaveGlow).run on the SAME buffers, alternating; the difference is what the stage
            costs a user, `stage_share_of_call` its share of the denoised call.

    python tools/denoise_bench.py [--json profiles/denoise_bench.json] [--seconds 0.5] [--repeats 3] [--shapes a,b] [--no-waveglow]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from glow_tts_amd import audio  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--json", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "denoise_bench.json"))
ap.add_argument("--seconds", type=float, default=0.5)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--shapes", default="single_1x800,batch_32x800", help="which shapes to run; an existing --json keeps its other shapes")
ap.add_argument("--no-waveglow", action="store_true", help="skip the WaveGlow graphs (3.2 GB of workspace at 32 x 800)")
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("denoise_bench needs the MI355X: there is nothing to time on a CPU")
dev = torch.device("cuda:0")
FRAMES, HOP, NFFT, CALLS, STRENGTH = 800, 256, 1024, 10, 0.1
T0 = time.time()


def say(*a):
    print(f"[{time.time() - T0:7.1f}s]", *a, flush=True)


def window(fn, per_call):
    """ms per call: `fn` (= per_call calls) repeated for >= args.seconds between two device events.  A single call that already
    fills the window is the measurement."""
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


def measure(variants):
    """{name: (fn, calls per fn)} -> ({name: best ms}, {name: every window}); the variants alternate inside every repeat"""
    times = {k: [] for k in variants}
    for _ in range(args.repeats):
        for k, (fn, per_call) in variants.items():
            times[k].append(window(fn, per_call))
            say(k, f"{times[k][-1]:.4f} ms")
    return {k: min(v) for k, v in times.items()}, times


# ---- the vocoder whose bias is subtracted: the published WaveGlow, random weights
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
den = audio.Denoiser.from_vocoder(voc, strength=STRENGTH)
wrapped = audio.Denoised(voc, denoiser=den)
torch.cuda.synchronize()
say("bias spectrum measured: max", float(den.bias_spec.max()))
fwd, inv, bias = den.stft.forward_basis, den.istft.inverse_basis, den.bias_spec


def envelope(n_frames):
    """the reference's window_sumsquare: a float32 buffer, each frame's float64 w^2 added in ascending frame order"""
    env = np.zeros(NFFT + HOP * (n_frames - 1), dtype=np.float32)
    w2 = audio.hann_periodic(NFFT) ** 2
    for f in range(n_frames):
        env[f * HOP:f * HOP + NFFT] += w2
    return torch.from_numpy(env).to(dev)


ENV = envelope(FRAMES + 1)
NONZERO = ENV > torch.finfo(torch.float32).tiny


def torch_denoise(y):
    x = F.pad(y.unsqueeze(1).unsqueeze(1), (NFFT // 2, NFFT // 2, 0, 0), mode="reflect").squeeze(1)
    ft = F.conv1d(x, fwd, stride=HOP)
    re, im = ft[:, :513], ft[:, 513:]
    mag, phase = torch.sqrt(re ** 2 + im ** 2), torch.atan2(im, re)
    mag = torch.clamp(mag - STRENGTH * bias[None, :, None], min=0.0)
    Bn, _, n = mag.shape
    frames = torch.matmul(torch.cat([mag * torch.cos(phase), mag * torch.sin(phase)], 1).transpose(1, 2), inv[:, 0])
    out = frames.new_zeros(Bn, n + 3, HOP)
    for q in range(NFFT // HOP):
        out[:, q:q + n] += frames[:, :, q * HOP:(q + 1) * HOP]
    out = out.view(Bn, 1, -1)
    out = torch.where(NONZERO, out / ENV, out) * (NFFT / HOP)
    return out[:, 0, NFFT // 2:-(NFFT // 2)]


result = {"device": torch.cuda.get_device_name(0), "frames_per_utterance": FRAMES, "strength": STRENGTH, "calls_per_replay": CALLS,
          "shapes": {}}
if os.path.exists(args.json):
    with open(args.json) as f:
        result["shapes"] = json.load(f).get("shapes", {})
for name, B in (("single_1x800", 1), ("batch_32x800", 32)):
    if name not in args.shapes.split(","):
        continue
    L = FRAMES * HOP
    y = torch.rand(B, L, generator=torch.Generator().manual_seed(B)).mul_(2).sub_(1).mul_(0.5).to(dev)
    n_frames = torch.full((B,), FRAMES, dtype=torch.int32, device=dev)
    bufs = den.workspace(B, FRAMES, dev)
    work = y.clone()
    den.run(work, n_frames, 0, bufs)
    want = torch_denoise(y)
    torch.cuda.synchronize()
    check = {"max_abs_diff": (work - want).abs().max().item(), "max_abs": want.abs().max().item(),
             "moved_by_the_stage": (want - y).abs().max().item()}
    say(name, "outputs", check)
    side = torch.cuda.Stream()
    g_spec, g_inv, g_pair = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(g_spec, stream=side):
        for _ in range(CALLS):
            den.analyse(y, n_frames, 0, bufs)
    with torch.cuda.graph(g_inv, stream=side):
        for _ in range(CALLS):
            den.istft.synthesize(bufs["dn_spec"], bufs["dn_frames"], B, FRAMES + 1, out=work)
    with torch.cuda.graph(g_pair, stream=side):
        for _ in range(CALLS):
            den.run(work, n_frames, 0, bufs)
    best, times = measure({"gt_denoise_spec": (g_spec.replay, CALLS), "gt_istft": (g_inv.replay, CALLS), "pair": (g_pair.replay, CALLS),
                           "torch": (lambda: torch_denoise(y), 1)})
    frames = B * (FRAMES + 1)
    shape = {"B": B, "audio_seconds_at_22050": B * L / 22050.0, "ms_best": best, "ms_windows": times, "outputs": check,
             "spec_gbps": frames * (4 * HOP + 4 * 1025 * 2) / best["gt_denoise_spec"] * 1e-6,
             "spec_tflops_issued": frames * 2.0 * 2 * 512 * 512 / best["gt_denoise_spec"] * 1e-9,
             "torch_over_pair": best["torch"] / best["pair"]}
    del g_spec, g_inv, g_pair, want
    if not args.no_waveglow:
        wb = wrapped.workspace(B, FRAMES, dev)
        mel = torch.randn(B, 80, FRAMES, generator=torch.Generator().manual_seed(2)).mul_(2.0).sub_(5.0).to(dev)
        seed_dev = torch.tensor([1], dtype=torch.int32, device=dev)
        voc.run(mel, n_frames, wb, seed_dev=seed_dev)
        wrapped.run(mel, n_frames, wb, seed_dev=seed_dev)
        torch.cuda.synchronize()
        g_plain, g_den = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with torch.cuda.graph(g_plain, stream=side):
            voc.run(mel, n_frames, wb, seed_dev=seed_dev)
        with torch.cuda.graph(g_den, stream=side):
            wrapped.run(mel, n_frames, wb, seed_dev=seed_dev)
        wbest, wtimes = measure({"waveglow": (g_plain.replay, 1), "denoised_waveglow": (g_den.replay, 1)})
        shape["waveglow"] = {"ms_best": wbest, "ms_windows": wtimes, "launches": [voc.launches, wrapped.launches],
                             "workspace_bytes": [voc.workspace_bytes(B, FRAMES), wrapped.workspace_bytes(B, FRAMES)],
                             "stage_ms_by_difference": wbest["denoised_waveglow"] - wbest["waveglow"],
                             "stage_share_of_call": best["pair"] / wbest["denoised_waveglow"]}
        del g_plain, g_den, wb
    result["shapes"][name] = shape
    print(name, json.dumps(shape), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:                                                   # after every shape: a later failure keeps the earlier one
        json.dump(result, f, indent=1)
print("wrote", args.json)
