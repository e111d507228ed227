"""dev: time of the device DTW (csrc/dtw.hip: gt_dtw_f32) against the same recurrence in PyTorch-ROCm on the same
device, vectorised over anti-diagonals and the batch, and against the float64 oracle (tests/dtw64.py, plain loops) on one CPU thread.

Two cases: the bench batch (B = 32 utterances of 800 x 760 frames) and ONE such utterance; features are tests/dtw64.py's warped
pairs (K = 13, padded to 16), alpha = 10 sqrt(2) / ln 10.  Per case:
  kernel    metrics.dtw (the DP launch and the walk-back launch) captured CALLS times in one graph and replayed; device events around
            >= --seconds of replays with a synchronise behind them, --repeats windows, the best and every window recorded.
  torch     the frame distances by one broadcast expression, skewed once so that anti-diagonal s is a row ([B, Fa + Fb - 1, Fa]),
            then Fa + Fb - 1 steps of three shifted minima: cost only — no direction bits, no path (the kernel's time includes both).
            Captured in a graph of its own and replayed in the same windows, alternating with the kernel.
  oracle    dtw64 on ONE utterance, one thread, once; the batch figure is 32 times that.
The costs of kernel and torch are compared once per case (max relative difference), so a fast wrong variant cannot pass unnoticed.
The split between the DP and the walk back is not taken here: it is the two kernels of a `rocprofv3 --kernel-trace --stats` run of
its own (--trace-only: a few eager calls of the batch case and nothing else).

    python tools/dtw_bench.py [--json profiles/dtw_bench.json] [--seconds 0.5] [--repeats 3] [--no-oracle] [--trace-only]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import dtw64 as R  # noqa: E402
from glow_tts_amd import metrics  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "dtw_bench.json"))
ap.add_argument("--seconds", type=float, default=0.5)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--no-oracle", action="store_true")
ap.add_argument("--trace-only", action="store_true")
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("dtw_bench needs the MI355X: there is nothing to time on a CPU")
dev = torch.device("cuda:0")
FA, FB, K, CALLS = 800, 760, 13, 5
ALPHA = float(np.float32(R.ALPHA_DB))


def make(B):
    pairs = [R.warped_pair(FA, FB, K, 1000 + i) for i in range(B)]
    a = torch.from_numpy(np.stack([p[0] for p in pairs])).to(dev)
    b = torch.from_numpy(np.stack([p[1] for p in pairs])).to(dev)
    a, b = torch.nn.functional.pad(a, (0, 16 - K)).contiguous(), torch.nn.functional.pad(b, (0, 16 - K)).contiguous()
    return pairs, a, b, torch.full((B,), FA, dtype=torch.int32, device=dev), torch.full((B,), FB, dtype=torch.int32, device=dev)


def skew_index(Fa, Fb, device):
    """(valid [Fa, S], column [Fa, S]) of row i on anti-diagonal s = i + j"""
    j = torch.arange(Fa + Fb - 1, device=device)[None, :] - torch.arange(Fa, device=device)[:, None]
    return (j >= 0) & (j < Fb), j.clamp(0, Fb - 1)


def torch_dtw(a, b, index, alpha):
    """cost [B] by anti-diagonals.  Slot i + 1 of a diagonal's vector is row i (slot 0: the row above the lattice, +inf):
    cur[i] = d[i, s - i] + min(prev2[i - 1] (diagonal), prev1[i - 1] ((i-1, j)), prev1[i] ((i, j-1)))"""
    B, Fa, Fb = a.shape[0], a.shape[1], b.shape[1]
    valid, col = index
    inf = float("inf")
    d = alpha * (a[:, :, None, :] - b[:, None, :, :]).pow(2).sum(-1).sqrt()          # [B, Fa, Fb]
    sk = d.gather(2, col[None].expand(B, -1, -1)).masked_fill(~valid[None], inf).transpose(1, 2).contiguous()   # [B, S, Fa]
    infcol = torch.full((B, 1), inf, device=a.device)
    prev2 = torch.full((B, Fa + 1), inf, device=a.device)
    prev1 = torch.full((B, Fa + 1), inf, device=a.device)
    prev2[:, 0] = 0.0                                                                  # D(-1, -1) = 0 makes D(0, 0) = d(0, 0)
    for s in range(Fa + Fb - 1):
        best = torch.minimum(torch.minimum(prev2[:, :-1], prev1[:, :-1]), prev1[:, 1:])
        prev2, prev1 = prev1, torch.cat([infcol, sk[:, s] + best], dim=1)
    return prev1[:, Fa]                                                               # D(Fa - 1, Fb - 1) sits on the last anti-diagonal


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


if args.trace_only:
    _, a, b, la, lb = make(32)
    for _ in range(5):
        metrics.dtw(a, la, b, lb, scale=ALPHA)
    torch.cuda.synchronize()
    sys.exit(0)

result = {"device": torch.cuda.get_device_name(0), "frames_a": FA, "frames_b": FB, "features": K, "alpha": ALPHA,
          "cells_per_utterance": FA * FB, "graph_calls_per_replay": CALLS, "cases": {}}
oracle_ms = None
if not args.no_oracle:
    x, y = R.warped_pair(FA, FB, K, 1000)
    d = R.dist64(x, y, ALPHA)
    t0 = time.perf_counter()
    R.dtw64(d)
    oracle_ms = (time.perf_counter() - t0) * 1e3
    result["oracle_float64_one_thread_ms_per_utterance"] = oracle_ms

for name, B in (("batch_32x800x760", 32), ("single_1x800x760", 1)):
    pairs, a, b, la, lb = make(B)
    res = metrics.dtw(a, la, b, lb, scale=ALPHA)
    index = skew_index(FA, FB, dev)
    want = torch_dtw(a, b, index, ALPHA)
    torch.cuda.synchronize()
    diff = ((res.cost - want).abs() / want).max().item()
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        for _ in range(CALLS):
            out = metrics.dtw(a, la, b, lb, scale=ALPHA)
    side2, graph2 = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph2, stream=side2):
        out2 = torch_dtw(a, b, index, ALPHA)
    variants = {"kernel": (graph.replay, CALLS), "torch_antidiagonals": (graph2.replay, 1)}
    times = {k: [] for k in variants}
    for _ in range(args.repeats):                                                     # the variants alternate inside every repeat
        for k, (fn, per_call) in variants.items():
            times[k].append(window(fn, per_call))
    best = {k: min(v) for k, v in times.items()}
    case = {"B": B, "ms_per_call_best": best, "ms_per_call_windows": times, "max_rel_diff_cost_torch_vs_kernel": diff,
            "mean_path_len": res.path_len.float().mean().item(),
            "kernel_cells_per_us": B * FA * FB / best["kernel"] * 1e-3,
            "torch_antidiagonals_over_kernel": best["torch_antidiagonals"] / best["kernel"]}
    if oracle_ms is not None:
        case["oracle_one_thread_over_kernel"] = oracle_ms * B / best["kernel"]
    result["cases"][name] = case
    print(name, json.dumps(case), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:                                                   # after every case: a later failure keeps the earlier one
        json.dump(result, f, indent=1)
print("wrote", args.json)
