"""dev: time of the Vocos vocoder (audio.Vocos on csrc/vocos.hip, gt_voc_conv and gt_istft) against the same model and
weights written with PyTorch-ROCm's own conv1d / layer_norm / linear / gelu / torch.istft on the same device.

Two shapes, the published model (80 bands, 512 / 1536 / 8 layers) with random weights: the bench batch (B = 32 utterances of 800 frames)
and ONE 800-frame utterance.  Per shape:
  kernel      Vocos.run (22 launches) captured in one graph and replayed; device events around >= --seconds of replays with a
              synchronise behind them, --repeats windows, the best and every window recorded.  The single utterance rotates over three
              workspaces and mels (one workspace alone would sit in the 256 MB Infinity Cache).
  kernels     every launch kind as a graph of its own — embed, the first norm, the L block norms, the L MLPs (out of place, so that
              replays do not grow the residual stream), the final norm, the head Linear, polar, istft: time per launch, the bytes an
              ideal launch moves (inputs and outputs once, the weight images once) with their share of the measured HBM copy rate, and
              for gt_vocos_mlp the achieved bf16 MFMA rate (4 C H FLOP per position).
  two_launch  the block's two products as two plain gt_voc_conv launches (taps 1: C -> H with bf16 out, H -> C with res), NO GELU
              between them: a yardstick built from kernels that already exist, for what keeping u on the chip is worth.
  torch       the published model in eager PyTorch on the padded batch (all utterances have one length), fp32 and under bf16
              autocast, alternating with the kernel in every repeat.
Outputs are compared once per shape: relative L2 of the kernel path and of the bf16 torch path against the fp32 torch result.

    python tools/vocos_bench.py [--json profiles/vocos_bench.json] [--seconds 0.5] [--repeats 3] [--shapes a,b]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from glow_tts_amd import _lib, audio  # noqa: E402
from glow_tts_amd._lib import call  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--json", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "vocos_bench.json"))
ap.add_argument("--seconds", type=float, default=0.5)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--shapes", default="single_1x800,batch_32x800", help="which shapes to run; an existing --json keeps its other shapes")
ap.add_argument("--no-torch", action="store_true", help="skip the PyTorch formulations")
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("vocos_bench needs the MI355X: there is nothing to time on a CPU")
dev = torch.device("cuda:0")
FRAMES, PEAK_BF16, HBM = 800, 2.5e15, 6.29e12
torch.manual_seed(0)
voc = audio.Vocos().to(dev)
with torch.no_grad():
    for blk in voc.backbone.convnext:
        blk.gamma.uniform_(0.1, 1.0)
C, H, NL = voc.dim, voc.intermediate_dim, voc.num_layers


def torch_vocos(mel):
    """the published model on the module's own fp32 parameters"""
    bb = voc.backbone
    ln = lambda x, m: F.layer_norm(x.transpose(1, 2), (C,), m.weight, m.bias, 1e-6)  # noqa: E731
    x = ln(F.conv1d(mel, bb.embed.weight, bb.embed.bias, padding=3), bb.norm).transpose(1, 2)
    for blk in bb.convnext:
        y = ln(F.conv1d(x, blk.dwconv.weight, blk.dwconv.bias, padding=3, groups=C), blk.norm)
        y = blk.gamma * F.linear(F.gelu(F.linear(y, blk.pwconv1.weight, blk.pwconv1.bias)), blk.pwconv2.weight, blk.pwconv2.bias)
        x = x + y.transpose(1, 2)
    o = F.linear(ln(x, bb.final_layer_norm), voc.head.out.weight, voc.head.out.bias).transpose(1, 2).float()
    mag, p = o.chunk(2, dim=1)
    mag = torch.clip(torch.exp(mag), max=1e2)
    return torch.istft(mag * (torch.cos(p) + 1j * torch.sin(p)), 1024, 256, 1024, torch.hann_window(1024, device=mel.device), center=True)


def torch_bf16(mel):
    with torch.autocast("cuda", dtype=torch.bfloat16):
        return torch_vocos(mel).float()


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


def kernel_launches(B, mel, n_frames, w, y2, u_ws):
    """{kind: (launch function, launches, ideal bytes per launch, FLOP per launch)} on one workspace"""
    im = voc.images()
    st = lambda: _lib.current_stream(dev)  # noqa: E731    the stream of the CALL: a capture's side stream
    Fr, sb, E = FRAMES, FRAMES * C, B * FRAMES * C
    x, a_, o, spec, wav = w["x"], w["a"], w["o"], w["spec"], w["wav"]

    def conv(X, img, Y, Cin, N, taps, x_sb, y_sb, res=None, **kw):
        call.gt_voc_conv(_lib.fill_args(_lib.VocConvArgs, X=X, x_stride_b=x_sb, W=img[0], bias=img[1], res=res, acc=None, Y=Y, y_stride_b=y_sb,
                                        ldy=N, len_mul=1, n_frames=n_frames, B=B, L_cap=Fr, Cin=Cin, N=N, taps=taps, dil=1, tanh_out=0,
                                        slope=1.0, scale=1.0, **kw), st())

    def norm(gb, Y, y_bf16, wd=None, bd=None):
        call.gt_vocos_norm(_lib.fill_args(_lib.VocosNormArgs, X=x, x_stride_b=sb, wd=wd, bd=bd, g=gb[0], be=gb[1], Y=Y, y_stride_b=sb,
                                          n_frames=n_frames, B=B, L_cap=Fr, C=C, y_bf16=y_bf16, eps=1e-6), st())

    def mlp(blk):
        call.gt_vocos_mlp(_lib.fill_args(_lib.VocosMlpArgs, A=a_, a_stride_b=sb, W1=blk["W1"], b1=blk["b1"], W2=blk["W2"], b2=blk["b2"], R=x,
                                         r_stride_b=sb, Y=y2, y_stride_b=sb, U=None, u_stride_b=0, n_frames=n_frames, B=B, L_cap=Fr, C=C, H=H), st())

    def two(blk):
        conv(a_, (blk["W1"], blk["b1"]), u_ws, C, H, 1, sb, Fr * H, x_stride_c=0, x_mel=0, x_bf16=1, y_bf16=1)
        conv(u_ws, (blk["W2"], blk["b2"]), y2, H, C, 1, Fr * H, sb, res=x, x_stride_c=0, x_mel=0, x_bf16=1, y_bf16=0)

    each = lambda f: (lambda: [f(blk) for blk in im["blocks"]])  # noqa: E731
    wimg = 2 * C * H * 2
    spec_b = spec.numel() * 4
    return {
        "embed": (lambda: conv(mel, im["embed"], x, 80, C, 7, mel.stride(0), sb, x_stride_c=mel.stride(1), x_mel=1, x_bf16=0, y_bf16=0), 1,
                  B * Fr * (80 + C) * 4 + im["embed"][0].numel() * 2, 2.0 * B * Fr * 7 * 80 * C),
        "norm_first": (lambda: norm(im["norm"], x, 0), 1, 8 * E, 0.0),
        "norm_block": (each(lambda blk: norm((blk["g"], blk["b"]), a_, 1, wd=blk["wd"], bd=blk["bd"])), NL, 6 * E, 0.0),
        "mlp": (each(mlp), NL, 10 * E + wimg, 4.0 * B * Fr * C * H),
        "norm_final": (lambda: norm(im["final"], a_, 1), 1, 6 * E, 0.0),
        "head": (lambda: conv(a_, im["head"], o, C, 1026, 1, sb, Fr * 1026, x_stride_c=0, x_mel=0, x_bf16=1, y_bf16=0), 1,
                 2 * E + B * Fr * 1026 * 4 + im["head"][0].numel() * 2, 2.0 * B * Fr * C * 1026),
        "polar": (lambda: call.gt_vocos_polar(_lib.fill_args(_lib.VocosPolarArgs, O=o, o_stride_b=Fr * 1026, n_frames=n_frames, spec=spec,
                                                             B=B, F_max=Fr, n_fft=1024), st()), 1, B * Fr * 1026 * 4 + spec_b, 0.0),
        "istft": (lambda: voc.istft.synthesize(spec, n_frames, B, Fr, out=wav), 1, spec_b + wav.numel() * 4, 0.0),
        "two_launch_products": (each(two), NL, 10 * E + wimg + 4 * B * Fr * H, 4.0 * B * Fr * C * H),
    }


T0 = time.time()
result = {"device": torch.cuda.get_device_name(0), "frames_per_utterance": FRAMES, "launches": voc.launches, "dim": C, "intermediate_dim": H,
          "num_layers": NL, "tile_positions": call.gt_vocos_tile_positions(), "hidden_chunk": call.gt_vocos_hidden_chunk(),
          "mlp_lds_bytes": call.gt_vocos_mlp_lds_bytes(C), "peak_bf16_flops": PEAK_BF16, "hbm_bytes_per_s": HBM,
          "hifigan_v1_recorded_ms": {"batch_32x800": 45.6, "single_1x800": 3.48}, "shapes": {}}
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
    say(name, f"inputs ready, workspace {voc.workspace_bytes(B, FRAMES) / 1e6:.1f} MB x {rot}")
    out_k = voc.run(mels[0], n_frames, works[0]).clone()
    torch.cuda.synchronize()
    say("kernel path ran once")
    side = torch.cuda.Stream()
    g_all = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g_all, stream=side):
        for m, w in zip(mels, works):
            voc.run(m, n_frames, w)
    y2 = [torch.empty(B * FRAMES * C, dtype=torch.float32, device=dev) for _ in range(rot)]
    u_ws = [torch.empty(B * FRAMES * H, dtype=torch.bfloat16, device=dev) for _ in range(rot)]
    kinds = [kernel_launches(B, m, n_frames, w, y, u) for m, w, y, u in zip(mels, works, y2, u_ws)]
    graphs = {}
    for kind in kinds[0]:
        for k in kinds:
            k[kind][0]()                                                              # once outside a capture
        graphs[kind] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[kind], stream=side):
            for k in kinds:
                k[kind][0]()
    for m, w in zip(mels, works):                                                     # the per-kind runs left the buffers in their run state
        voc.run(m, n_frames, w)
    torch.cuda.synchronize()
    times = {}

    def measure(variants):
        for _ in range(args.repeats):                                                 # the variants alternate inside every repeat
            for k, (fn, per_call) in variants.items():
                times.setdefault(k, []).append(window(fn, per_call))
                say(k, f"{times[k][-1]:.4f} ms")

    def record(check):
        best = {k: min(v) for k, v in times.items()}
        per_kernel = {}
        for kind, (_, n, nbytes, flop) in kinds[0].items():
            ms = best[kind] / n
            per_kernel[kind] = {"launches": n, "ms_per_launch": ms, "ms_total": best[kind], "mbytes_per_launch": nbytes * 1e-6,
                                "share_of_hbm_rate": nbytes / HBM * 1e3 / ms}
            if flop:
                per_kernel[kind].update(gflop_per_launch=flop * 1e-9, tflops=flop / ms * 1e-9, share_of_bf16_peak=flop / PEAK_BF16 * 1e3 / ms)
        own = [k for k in kinds[0] if k != "two_launch_products"]
        shape = {"B": B, "audio_seconds_at_22050": B * (FRAMES - 1) * 256 / 22050.0, "workspace_mbytes": voc.workspace_bytes(B, FRAMES) * 1e-6,
                 "ms_best": best, "ms_windows": times, "outputs": check, "kernels": per_kernel,
                 "kernel_sum_share_of_run": sum(best[k] for k in own) / best["kernel"],
                 "fused_mlp_over_two_launches": best["mlp"] / best["two_launch_products"],
                 "real_time_factor": B * (FRAMES - 1) * 256 / 22050.0 / (best["kernel"] * 1e-3),
                 "hifigan_v1_recorded_over_kernel": result["hifigan_v1_recorded_ms"][name] / best["kernel"]}
        for k in ("torch_fp32", "torch_bf16_autocast"):
            shape[k + "_over_kernel"] = best[k] / best["kernel"] if k in best else "not measured"
        result["shapes"][name] = shape
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:                                               # after every phase: a later failure keeps the earlier one
            json.dump(result, f, indent=1)
        return shape

    variants = {"kernel": (g_all.replay, rot)}
    variants.update({k: (gr.replay, rot) for k, gr in graphs.items()})
    measure(variants)
    shape = record({})
    if not args.no_torch:
        with torch.no_grad():
            out_t = torch_vocos(mels[0])
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
                torch_vocos(mels[rr[0] % rot])

        def t16():
            with torch.no_grad():
                rr[0] += 1
                torch_bf16(mels[rr[0] % rot])
        measure({"kernel": (g_all.replay, rot), "torch_fp32": (t32, 1), "torch_bf16_autocast": (t16, 1)})
        shape = record(check)
    print(name, json.dumps(shape), flush=True)
    del works, graphs, g_all, kinds, y2, u_ws
print("wrote", args.json)
