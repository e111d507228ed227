"""dev: time of the device resampler (csrc/resample.hip) against the same filter bank as a strided conv1d in
PyTorch-ROCm on the same device, and against scipy.signal.resample_poly on one CPU thread.

48 000 -> 22 050 Hz, int16 in.  Two shapes: the bench batch (B = 32 utterances of 445 544 samples = 9.28 s each, whose 204 672 outputs
are the utterance of tools/mel_bench.py) and ONE such utterance.  Per shape:
  kernel    audio.Resample.transform captured CALLS times in one graph and replayed; device events around >= --seconds of replays with
            a synchronise behind them, --repeats windows, the best and every window recorded.
  torch     eager: output n = m up + r is channel r of a conv1d of stride `down` over the zero-padded fp32 waveform, its kernel the
            bank row of phase (r down + half) mod up placed at that channel's input offset (a [up, 1, K] weight, K = 383, built
            once), then a transpose to sample order.  Same windows, alternating with the kernel.
  scipy     resample_poly(x, 147, 320) on ONE utterance in float32 -> float64 arithmetic as scipy does it, best of three calls, one
            thread (scipy's upfirdn has no other); the batch figure is 32 times that.
HBM floor: 2 bytes per input sample + 4 per output sample over 8.0 TB/s (the spec peak; 6.29 TB/s is what a copy measures).
The outputs of kernel and conv1d are compared once per shape (max |difference|), so a fast wrong variant cannot pass unnoticed.

    python tools/resample_bench.py [--json profiles/resample_bench.json] [--seconds 0.5] [--repeats 3] [--no-scipy]"""
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
ap.add_argument("--json", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "resample_bench.json"))
ap.add_argument("--seconds", type=float, default=0.5)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--no-scipy", action="store_true")
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("resample_bench needs the MI355X: there is nothing to time on a CPU")
dev = torch.device("cuda:0")
ORIG, NEW, L, CALLS, HBM_SPEC, HBM_COPY = 48000, 22050, 445544, 10, 8.0e12, 6.29e12
mod = audio.Resample(ORIG, NEW).to(dev)
up, down, T = mod.up, mod.down, mod.taps
N_OUT = mod.out_len(L)
half = 10 * max(up, down)

# the bank as ONE strided convolution: channel r = outputs n = m up + r, reading x[m down + c_r - j] for tap j of phase p_r
r = np.arange(up)
p_r, c_r = (r * down + half) % up, (r * down + half) // up
K = int(c_r.max()) + T
w = np.zeros((up, K), dtype=np.float32)
bank = mod.bank.cpu().numpy()
for ch in range(up):
    w[ch, c_r[ch] + (T - 1) - np.arange(T)] = bank[p_r[ch]]
weight = torch.from_numpy(w)[:, None, :].to(dev)
M = -(-N_OUT // up)


def torch_conv1d(y):
    x = F.pad(y.float() / 32768.0, (T - 1, (M - 1) * down + K - (T - 1) - y.shape[1]))
    return F.conv1d(x[:, None, :], weight, stride=down).transpose(1, 2).reshape(y.shape[0], -1)[:, :N_OUT]


def window(fn, per_call):
    """ms per call: `fn` (= per_call calls) repeated for >= args.seconds between two device events"""
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


result = {"device": torch.cuda.get_device_name(0), "orig_freq": ORIG, "new_freq": NEW, "up": up, "down": down, "taps": T,
          "samples_in_per_utterance": L, "samples_out_per_utterance": N_OUT, "graph_calls_per_replay": CALLS, "conv1d_kernel_width": K,
          "hbm_bytes_per_s_spec": HBM_SPEC, "hbm_bytes_per_s_copy": HBM_COPY, "shapes": {}}
scipy_ms = None
if not args.no_scipy:
    from scipy import signal
    x1 = np.random.default_rng(1).integers(-32768, 32768, L).astype(np.float32) / np.float32(32768.0)
    best = float("inf")
    for _ in range(3):
        t0 = time.perf_counter()
        signal.resample_poly(x1, up, down)
        best = min(best, time.perf_counter() - t0)
    scipy_ms = best * 1e3
    result["scipy_one_thread_ms_per_utterance"] = scipy_ms

for name, B in (("batch_32x9.28s", 32), ("single_1x9.28s", 1)):
    y = torch.randint(-32768, 32768, (B, L), generator=torch.Generator().manual_seed(B), dtype=torch.int32).to(torch.int16).to(dev)
    ln = torch.full((B,), L, dtype=torch.int32, device=dev)
    out_k, _ = mod.transform(y, ln, N_OUT)
    torch.cuda.synchronize()
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        for _ in range(CALLS):
            out = mod.transform(y, ln, N_OUT)
    variants = {"kernel": (graph.replay, CALLS), "torch_conv1d": (lambda: torch_conv1d(y), 1)}
    diff = (torch_conv1d(y) - out_k).abs().max().item()
    times = {k: [] for k in variants}
    for _ in range(args.repeats):                                                     # the variants alternate inside every repeat
        for k, (fn, per_call) in variants.items():
            times[k].append(window(fn, per_call))
    best = {k: min(v) for k, v in times.items()}
    nbytes = B * (2.0 * L + 4.0 * N_OUT)
    floor_ms = nbytes / HBM_SPEC * 1e3
    shape = {"B": B, "ms_per_call_best": best, "ms_per_call_windows": times, "max_abs_diff_conv1d_vs_kernel": diff,
             "hbm_bytes": nbytes, "hbm_floor_ms_at_spec": floor_ms, "kernel_fraction_of_hbm_floor": floor_ms / best["kernel"],
             "kernel_fraction_of_copy_rate": nbytes / HBM_COPY * 1e3 / best["kernel"],
             "kernel_gflops": B * N_OUT * 2.0 * T / best["kernel"] * 1e-6,
             "kernel_seconds_of_audio_per_ms": B * L / ORIG / best["kernel"],
             "torch_conv1d_over_kernel": best["torch_conv1d"] / best["kernel"]}
    if scipy_ms is not None:
        shape["scipy_one_thread_over_kernel"] = scipy_ms * B / best["kernel"]
    result["shapes"][name] = shape
    print(name, json.dumps(shape), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:                                                   # after every shape: a later failure keeps the earlier one
        json.dump(result, f, indent=1)
print("wrote", args.json)
