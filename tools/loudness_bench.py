"""dev: time of the BS.1770 loudness stage (audio.Loudness on csrc/loudness.hip) against the HBM floor, against the same
definition in scipy on one CPU thread, and as a share of a Vocos and a WaveGlow call.

  stage     Loudness.run's two C-ABI calls captured in graphs and replayed — gt_loudness_measure alone (four launches),
            gt_loudness_apply alone (one) and the pair (10 calls a replay) — on 800-frame utterances of 256-sample hops (204 800
            samples, 9.3 s at 22 050 Hz), one of them and a batch of 32.
  floor     x read twice, y written once (12 bytes a sample) at HBM_PEAK_TBPS; `pair_gbps` is what the pair reaches of those bytes.
            (The 26 MB of the batch fit the 256 MB Infinity Cache: a rate above HBM's is no error.)
  scipy     scipy.signal.lfilter twice, the segment sums, blocks and both gates in NumPy, utterance by utterance on one thread.
  vocoders  the graph of Vocos.run and of WaveGlow.run (random weights: the time does not depend on them) at the same capacity;
            `stage_share_of_call` is pair / (vocoder + pair).  The vocoders' code is the parent commit's.

    python tools/loudness_bench.py [--json profiles/loudness_bench.json] [--seconds 0.5] [--repeats 3] [--shapes a,b] [--no-vocoders]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from glow_tts_amd import audio  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--json", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "loudness_bench.json"))
ap.add_argument("--seconds", type=float, default=0.5)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--shapes", default="single_1x800,batch_32x800", help="which shapes to run; an existing --json keeps its other shapes")
ap.add_argument("--no-vocoders", action="store_true", help="skip the Vocos and WaveGlow graphs (3.2 GB of workspace at 32 x 800)")
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("loudness_bench needs the MI355X: there is nothing to time on a CPU")
dev = torch.device("cuda:0")
FRAMES, HOP, FS, CALLS, HBM_PEAK_TBPS = 800, 256, 22050, 10, 8.0
T0 = time.time()


def say(*a):
    print(f"[{time.time() - T0:7.1f}s]", *a, flush=True)


def window(fn, per_call):
    """ms per call: `fn` (= per_call calls) repeated for >= args.seconds between two device events"""
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


def scipy_loudness(x, fs=FS):
    """the definition on the host: -> L of one utterance (float64)"""
    from scipy.signal import lfilter
    (b, a), (c, d) = audio.kweighting64(fs)
    z = lfilter(c, d, lfilter(b, a, x.astype(np.float64)))
    Ns = fs // 10
    S = len(z) // Ns
    E = (z[:S * Ns].reshape(S, Ns) ** 2).sum(1)
    zj = (E[:-3] + E[1:-2] + E[2:-1] + E[3:]) / (4 * Ns)
    with np.errstate(divide="ignore"):
        l = -0.691 + 10 * np.log10(zj)
        A = l > -70.0
        if not A.any():
            return -np.inf
        R = A & (l > -0.691 + 10 * np.log10(zj[A].mean()) - 10.0)
        return -0.691 + 10 * np.log10(zj[R].mean())


def random_vocoder(voc):
    """random weights in the published shapes: the time does not depend on them"""
    with torch.no_grad():
        for p in voc.parameters():
            p.uniform_(-1.0, 1.0).mul_(1.0 / max(p[0].numel(), 1) ** 0.5 if p.dim() > 1 else 0.1)
    return voc.to(dev)


loud = audio.Loudness(FS).to(dev)
scipy_loudness(np.zeros(FS, dtype=np.float32))                                        # scipy's import is not what is timed
result = {"device": torch.cuda.get_device_name(0), "frames_per_utterance": FRAMES, "samples_per_utterance": FRAMES * HOP,
          "sampling_rate": FS, "chunk": loud.chunk, "calls_per_replay": CALLS, "hbm_peak_tbps": HBM_PEAK_TBPS, "shapes": {}}
if os.path.exists(args.json):
    with open(args.json) as f:
        result["shapes"] = json.load(f).get("shapes", {})
for name, B in (("single_1x800", 1), ("batch_32x800", 32)):
    if name not in args.shapes.split(","):
        continue
    N = FRAMES * HOP
    # speech-like levels: noise under a slow envelope that falls to silence, so that both gates have work
    g = torch.Generator().manual_seed(B)
    env = (0.5 + 0.5 * torch.sin(torch.arange(N) * (2 * np.pi / (FS * 1.7)))).clamp_min(0.0) ** 4
    y = (torch.rand(B, N, generator=g).mul_(2).sub_(1) * env * 0.5).to(dev)
    n_frames = torch.full((B,), FRAMES, dtype=torch.int32, device=dev)
    bufs = loud.workspace(B, FRAMES, dev, HOP, 0)
    work = y.clone()
    loud.run(work, n_frames, HOP, 0, bufs)
    torch.cuda.synchronize()
    stats = bufs["ld_stats"].view(B, 8).cpu().numpy()
    t0 = time.perf_counter()
    want = np.array([scipy_loudness(row) for row in y.cpu().numpy()])
    scipy_ms = (time.perf_counter() - t0) * 1e3
    check = {"max_abs_L_diff_vs_scipy": float(np.abs(stats[:, 0] - want).max()), "L_range": [float(want.min()), float(want.max())],
             "blocks": float(stats[0, 3]), "gated_abs": float(stats[:, 4].mean()), "gated_rel": float(stats[:, 5].mean())}
    say(name, "outputs", check, f"scipy {scipy_ms:.1f} ms")
    side = torch.cuda.Stream()
    st = audio._lib.current_stream
    g_meas, g_apply, g_pair = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    blk = loud._args(work, n_frames, HOP, 0, bufs)
    with torch.cuda.graph(g_meas, stream=side):
        for _ in range(CALLS):
            audio.call.gt_loudness_measure(blk, st(dev))
    with torch.cuda.graph(g_apply, stream=side):
        for _ in range(CALLS):
            audio.call.gt_loudness_apply(blk, st(dev))
    with torch.cuda.graph(g_pair, stream=side):
        for _ in range(CALLS):
            loud.run(work, n_frames, HOP, 0, bufs)
    best, times = measure({"gt_loudness_measure": (g_meas.replay, CALLS), "gt_loudness_apply": (g_apply.replay, CALLS),
                           "pair": (g_pair.replay, CALLS)})
    floor_ms = B * N * 12 / (HBM_PEAK_TBPS * 1e12) * 1e3
    shape = {"B": B, "audio_seconds_at_22050": B * N / float(FS), "ms_best": best, "ms_windows": times, "outputs": check,
             "hbm_floor_ms": floor_ms, "pair_over_floor": best["pair"] / floor_ms, "pair_gbps": B * N * 12 / best["pair"] * 1e-6,
             "scipy_one_thread_ms": scipy_ms, "scipy_over_measure": scipy_ms / best["gt_loudness_measure"],
             "workspace_bytes": int(bufs["ld_ws"].numel() * 4)}
    del g_meas, g_apply, g_pair
    if not args.no_vocoders:
        shape["vocoders"] = {}
        for vname, make, seeded in (("vocos", audio.Vocos, False), ("waveglow", audio.WaveGlow, True)):
            torch.manual_seed(0)
            voc = random_vocoder(make())
            wb = voc.workspace(B, FRAMES, dev)
            mel = torch.randn(B, voc.mel_channels, FRAMES, generator=torch.Generator().manual_seed(2)).mul_(2.0).sub_(5.0).to(dev)
            kw = dict(seed_dev=torch.tensor([1], dtype=torch.int32, device=dev)) if seeded else {}
            voc.run(mel, n_frames, wb, **kw)
            torch.cuda.synchronize()
            g_voc = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g_voc, stream=side):
                voc.run(mel, n_frames, wb, **kw)
            vbest, vtimes = measure({vname: (g_voc.replay, 1)})
            rows = wb["wav"].shape[1]
            shape["vocoders"][vname] = {"ms_best": vbest[vname], "ms_windows": vtimes[vname], "launches": voc.launches,
                                        "samples_per_row": rows,
                                        "stage_share_of_call": best["pair"] * rows / N / (vbest[vname] + best["pair"] * rows / N)}
            del g_voc, wb, voc
            torch.cuda.empty_cache()
    result["shapes"][name] = shape
    print(name, json.dumps(shape), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:                                                   # after every shape: a later failure keeps the earlier one
        json.dump(result, f, indent=1)
print("wrote", args.json)
