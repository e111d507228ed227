"""dev: time of the device mel front end (csrc/mel_front.hip) against the reference's formulation in PyTorch-ROCm on
the same device.

Two shapes: the bench batch (B = 32 utterances of 800 frames each = 204 672 samples) and one 800-frame utterance.  Per shape:
  kernel    audio.TacotronSTFT.transform (mel + energy, no magnitudes) captured CALLS times in one graph and replayed; device events
            around >= --seconds of replays with a synchronise behind them, --repeats windows, the best and every window recorded.
  torch     the reference's CUDA branch, eager: F.pad(reflect) -> F.conv1d(forward_basis, stride 256) -> sqrt(re^2 + im^2) ->
            matmul(mel_basis) -> log(clamp) and the norm over bins; and the same with the conv written as unfold + matmul (the fp32
            GEMM library), since the conv1d of a 1024-tap, 1026-channel filter is not a shape convolution libraries are tuned for.
            Same windows, the two alternating with the kernel.  All utterances of a shape have one length, so one batched call IS the
            per-utterance transform.
FLOP/s: `flops_dft` = 2 * 1024 * 1026 per frame, the unfolded DFT every formulation has to deliver (the rate a user compares);
`flops_issued` = what the kernel's MFMAs execute after the centre fold (2 * 2 * 512 * 512 for the DFT + 2 * 512 * 96 for the mel
projection per frame), whose share of the kernel guide's 122 TF/s untuned fp32-MFMA GEMM says how busy the matrix cores are.
The outputs of the three are compared once per shape (max |mel difference|), so a fast wrong variant cannot pass unnoticed.

    python tools/mel_bench.py [--json profiles/mel_front_bench.json] [--seconds 0.5] [--repeats 3] [--no-conv1d]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from glow_tts_amd import audio  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--json", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "mel_front_bench.json"))
ap.add_argument("--seconds", type=float, default=0.5)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--no-conv1d", action="store_true", help="skip the F.conv1d form (keep unfold + matmul)")
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("mel_bench needs the MI355X: there is nothing to time on a CPU")
dev = torch.device("cuda:0")
FRAMES, HOP, NFFT, CALLS, GUIDE_TFLOPS = 800, 256, 1024, 10, 122.0
mod = audio.TacotronSTFT().to(dev)


def torch_conv1d(y):
    x = F.pad(y.unsqueeze(1).unsqueeze(1), (NFFT // 2, NFFT // 2, 0, 0), mode="reflect").squeeze(1)
    ft = F.conv1d(x, mod.stft_fn.forward_basis, stride=HOP)
    mag = torch.sqrt(ft[:, :513] ** 2 + ft[:, 513:] ** 2)
    return torch.log(torch.clamp(torch.matmul(mod.mel_basis, mag), min=audio.CLIP_VAL)), torch.norm(mag, dim=1)


def torch_unfold(y):
    x = F.pad(y.unsqueeze(1).unsqueeze(1), (NFFT // 2, NFFT // 2, 0, 0), mode="reflect").squeeze(1).squeeze(1)
    ft = torch.matmul(x.unfold(1, NFFT, HOP), mod.stft_fn.forward_basis[:, 0].t()).transpose(1, 2)
    mag = torch.sqrt(ft[:, :513] ** 2 + ft[:, 513:] ** 2)
    return torch.log(torch.clamp(torch.matmul(mod.mel_basis, mag), min=audio.CLIP_VAL)), torch.norm(mag, dim=1)


def window(fn, per_call):
    """ms per transform: `fn` (= per_call transforms) repeated for >= args.seconds between two device events"""
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
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


result = {"device": torch.cuda.get_device_name(0), "frames_per_utterance": FRAMES, "graph_calls_per_replay": CALLS,
          "guide_fp32_mfma_gemm_tflops": GUIDE_TFLOPS, "shapes": {}}
for name, B in (("batch_32x800", 32), ("single_1x800", 1)):
    L = (FRAMES - 1) * HOP + 128
    y = torch.rand(B, L, generator=torch.Generator().manual_seed(B)).mul_(2).sub_(1).to(dev)
    ln = torch.full((B,), L, dtype=torch.int32, device=dev)
    mel_k, en_k, _ = mod.transform(y, ln, FRAMES)
    torch.cuda.synchronize()
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        for _ in range(CALLS):
            out = mod.transform(y, ln, FRAMES)
    variants = {"kernel": (graph.replay, CALLS), "torch_unfold_matmul": (lambda: torch_unfold(y), 1)}
    if not args.no_conv1d:
        variants["torch_conv1d"] = (lambda: torch_conv1d(y), 1)
    diffs = {}
    for k, (fn, _) in variants.items():
        if k != "kernel":
            mel_t, en_t = fn()
            diffs[k] = {"max_abs_mel_diff": (mel_t - mel_k).abs().max().item(), "max_rel_energy_diff": ((en_t - en_k).abs() / en_k).max().item()}
    times = {k: [] for k in variants}
    for _ in range(args.repeats):                                                     # the variants alternate inside every repeat
        for k, (fn, per_call) in variants.items():
            times[k].append(window(fn, per_call))
    frames = B * FRAMES
    best = {k: min(v) for k, v in times.items()}
    flops_dft, flops_issued = frames * 2.0 * NFFT * 1026, frames * (2.0 * 2 * 512 * 512 + 2.0 * 512 * 96)
    shape = {"B": B, "samples_per_utterance": L, "ms_per_call_best": best, "ms_per_call_windows": times, "outputs_vs_kernel": diffs,
             "kernel_tflops_dft_equivalent": flops_dft / best["kernel"] * 1e-9,
             "kernel_tflops_issued": flops_issued / best["kernel"] * 1e-9,
             "kernel_issued_share_of_guide_gemm": flops_issued / best["kernel"] * 1e-9 / GUIDE_TFLOPS,
             "kernel_mframes_per_s": frames / best["kernel"] * 1e-3}
    for k in variants:
        if k != "kernel":
            shape[f"{k}_over_kernel"] = best[k] / best["kernel"]
    result["shapes"][name] = shape
    print(name, json.dumps(shape), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:                                                   # after every shape: a later failure keeps the earlier one
        json.dump(result, f, indent=1)
print("wrote", args.json)
