"""dev: time of the device waveform back end (csrc/griffin_lim.hip) against the reference's formulation in
PyTorch-ROCm on the same device and the same inputs.

Two shapes: the bench batch (B = 32 utterances of 800 frames) and one 800-frame utterance.  Per shape:
  kernel    audio.GriffinLim's 30-iteration loop (gt_gl_polar, gt_istft, 30 x (gt_gl_project, gt_istft)) from fixed angles, captured
            in one graph and replayed; device events around >= --seconds of replays with a synchronise behind them, --repeats
            windows, the best and every window recorded.  Also the two MFMA kernels alone (10 calls per replay), for the roofline.
  torch     the reference's loop, eager: the inverse (cos / sin, the transposed convolution with inverse_basis at stride 256, the
            float32 squared-window envelope, * 4, trim); then per iteration F.pad(reflect) -> F.conv1d(forward_basis, stride 256)
            -> atan2 -> the inverse.  The transposed convolution is written as matmul + four shifted adds (the GEMM and the
            overlap-add it is), NOT as F.conv_transpose1d: on the stack this was measured on, F.conv_transpose1d with this
            1026-channel, 1024-tap filter did not return within four minutes for ONE 800-frame utterance.
            Same windows, alternating with the kernel.  All utterances of a shape have one length, so one batched call IS the
            per-utterance loop.
FLOP/s: `flops_dft` = 2 * 2 * 1024 * 1026 per frame and iteration, the unfolded forward + inverse DFT every formulation has to
deliver; `flops_issued` = what the MFMAs execute after the centre fold: 2 * 2 * 512 * 512 per frame for the analysis and, with the
3-frame halo of a 64-frame tile, 64 / 61 times that for the synthesis.
The two loops' outputs are compared once per shape by what Griffin-Lim is for — the spectral convergence of each end point, measured
by the SAME analysis (the eager one) — since 30 iterations of a phase retrieval started identically still end at different samples in
different arithmetic.  One inverse (no iteration) is compared sample by sample.

A torch loop call that alone fills a window is timed as that one call.  Progress lines carry the host's wall clock.

    python tools/gl_bench.py [--json profiles/griffin_lim_bench.json] [--seconds 0.5] [--repeats 3] [--iters 30] [--shapes a,b]"""
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
ap.add_argument("--json", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "griffin_lim_bench.json"))
ap.add_argument("--seconds", type=float, default=0.5)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--shapes", default="single_1x800,batch_32x800", help="which shapes to run; an existing --json keeps its other shapes")
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("gl_bench needs the MI355X: there is nothing to time on a CPU")
dev = torch.device("cuda:0")
FRAMES, HOP, NFFT, CALLS = 800, 256, 1024, 10
gl = audio.GriffinLim(audio.TacotronSTFT()).to(dev)
fwd, inv = gl.stft_fn.forward_basis, gl.istft.inverse_basis


def envelope(n_frames):
    """the reference's window_sumsquare: a float32 buffer, each frame's float64 w^2 added in ascending frame order"""
    env = np.zeros(NFFT + HOP * (n_frames - 1), dtype=np.float32)
    w2 = audio.hann_periodic(NFFT) ** 2
    for f in range(n_frames):
        env[f * HOP:f * HOP + NFFT] += w2
    return torch.from_numpy(env).to(dev)


ENV = envelope(FRAMES)
NONZERO = ENV > torch.finfo(torch.float32).tiny


def torch_inverse(mag, phase):
    """conv_transpose1d(recombined, inverse_basis, stride 256) written as the GEMM and the overlap-add it is: frames = Y^T ib, frame f
    added at sample 256 f (four shifted adds of the frames' quarters)"""
    B, _, n = mag.shape
    frames = torch.matmul(torch.cat([mag * torch.cos(phase), mag * torch.sin(phase)], 1).transpose(1, 2), inv[:, 0])
    x = frames.new_zeros(B, n + 3, HOP)
    for q in range(NFFT // HOP):
        x[:, q:q + n] += frames[:, :, q * HOP:(q + 1) * HOP]
    x = x.view(B, 1, -1)
    x = torch.where(NONZERO, x / ENV, x) * (NFFT / HOP)
    return x[:, 0, NFFT // 2:-(NFFT // 2)]


def torch_transform(y):
    x = F.pad(y.unsqueeze(1).unsqueeze(1), (NFFT // 2, NFFT // 2, 0, 0), mode="reflect").squeeze(1)
    ft = F.conv1d(x, fwd, stride=HOP)
    re, im = ft[:, :513], ft[:, 513:]
    return torch.sqrt(re ** 2 + im ** 2), torch.atan2(im, re)


def torch_loop(mag, angles, n):
    y = torch_inverse(mag, angles)
    for _ in range(n):
        _, ph = torch_transform(y)
        y = torch_inverse(mag, ph)
    return y


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


def convergence(y, mag):
    got, _ = torch_transform(y)
    return (torch.linalg.norm(got - mag) / torch.linalg.norm(mag)).item()


T0 = time.time()
result = {"device": torch.cuda.get_device_name(0), "frames_per_utterance": FRAMES, "iterations": args.iters,
          "tile_frames": audio.call.gt_gl_tile_frames(), "tile_hops": audio.call.gt_gl_tile_hops(), "shapes": {}}
if os.path.exists(args.json):
    with open(args.json) as f:
        result["shapes"] = json.load(f).get("shapes", {})
for name, B in (("single_1x800", 1), ("batch_32x800", 32)):
    if name not in args.shapes.split(","):
        continue
    L = (FRAMES - 1) * HOP
    y = torch.rand(B, L, generator=torch.Generator().manual_seed(B)).mul_(2).sub_(1).to(dev)
    mag, _ = torch_transform(y)
    mag = mag.contiguous()
    angles = torch.empty_like(mag).uniform_(-np.pi, np.pi, generator=torch.Generator(device=dev).manual_seed(1))
    n_frames = torch.full((B,), FRAMES, dtype=torch.int32, device=dev)
    say(name, "inputs ready")
    out_k = gl(mag, n_iters=args.iters, angles=angles)
    one_k = gl(mag, n_iters=0, angles=angles)
    torch.cuda.synchronize()
    say("kernel loop ran once")
    one_t = torch_inverse(mag, angles)
    torch.cuda.synchronize()
    say("torch inverse ran once")
    out_t = torch_loop(mag, angles, args.iters)
    torch.cuda.synchronize()
    say("torch loop ran once")
    check = {"one_inverse_max_abs_diff": (one_k - one_t).abs().max().item(), "one_inverse_max_abs": one_t.abs().max().item(),
             "convergence_kernel": convergence(out_k, mag), "convergence_torch": convergence(out_t, mag),
             "convergence_start": convergence(one_t, mag)}
    side = torch.cuda.Stream()
    g_loop, g_proj, g_inv = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(g_loop, stream=side):
        out = gl(mag, n_iters=args.iters, angles=angles)
    spec, wav = gl.istft.workspace(B, FRAMES, dev), out_k.clone()
    with torch.cuda.graph(g_proj, stream=side):
        for _ in range(CALLS):
            gl.project(wav, mag, n_frames, spec)
    with torch.cuda.graph(g_inv, stream=side):
        for _ in range(CALLS):
            gl.istft.synthesize(spec, n_frames, B, FRAMES, out=wav)
    variants = {"kernel_loop": (g_loop.replay, 1), "torch_loop": (lambda: torch_loop(mag, angles, args.iters), 1),
                "gt_gl_project": (g_proj.replay, CALLS), "gt_istft": (g_inv.replay, CALLS)}
    times = {k: [] for k in variants}
    for _ in range(args.repeats):                                                     # the variants alternate inside every repeat
        for k, (fn, per_call) in variants.items():
            times[k].append(window(fn, per_call))
            say(k, f"{times[k][-1]:.3f} ms")
    best = {k: min(v) for k, v in times.items()}
    frames = B * FRAMES
    fold = 2.0 * 2 * 512 * 512
    flops_dft = frames * args.iters * 2.0 * 2 * NFFT * 1026
    halo = result["tile_frames"] / result["tile_hops"]
    shape = {"B": B, "audio_seconds_at_22050": B * L / 22050.0, "ms_best": best, "ms_windows": times, "outputs": check,
             "loop_tflops_dft_equivalent": flops_dft / best["kernel_loop"] * 1e-9,
             "project_tflops_issued": frames * fold / best["gt_gl_project"] * 1e-9,
             "istft_tflops_issued": frames * fold * halo / best["gt_istft"] * 1e-9,
             "launch_sum_share_of_loop": (args.iters * best["gt_gl_project"] + (args.iters + 1) * best["gt_istft"]) / best["kernel_loop"],
             "torch_over_kernel": best["torch_loop"] / best["kernel_loop"]}
    result["shapes"][name] = shape
    print(name, json.dumps(shape), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:                                                   # after every shape: a later failure keeps the earlier one
        json.dump(result, f, indent=1)
print("wrote", args.json)
