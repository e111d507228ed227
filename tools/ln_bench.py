"""Micro-benchmark of the LayerNorm entries through the C-ABI, graph-replayed (dev tool).

    python tools/ln_bench.py [path/to/libglowtts_hip.so] [--sets N]

The encoder's shape at cfg 2 (28 utterances x 124 tokens, C = 192), the post-attention form: a + bf16 y with p_in = 0.1, both dout
forms, da and dy wanted.  Times gt_layernorm_fwd, gt_layernorm_bwd (atomics) and gt_layernorm_bwd_partials, three repeats each of
20 replays of a graph of 20 launches.  `warm`: the same operands every launch (they stay in L2); `rotating`: N operand sets (default
24, ~290 MB: past L2 and the 256 MB Infinity Cache) taken in turn, which is how the step sees the saved rows."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from glow_tts_amd import _lib
args = [a for a in sys.argv[1:] if not a.startswith("--")]
if args:
    _lib.LIB_PATH = os.path.abspath(args[0])
NSETS = int(sys.argv[sys.argv.index("--sets") + 1]) if "--sets" in sys.argv else 24
L, P = _lib.lib(), _lib.ptr
dev = torch.device("cuda:0")
R, C, EPS, N = 28 * 124, 192, 1e-4, 20
g = torch.Generator(device="cpu").manual_seed(0)
gam, beta = (1 + 0.1 * torch.randn(C, generator=g)).to(dev), (0.1 * torch.randn(C, generator=g)).to(dev)
rm = torch.ones(R, device=dev)
word = torch.tensor([7], dtype=torch.int32, device=dev)


def make_set():
    s = {"a": torch.randn(R, C, device=dev), "y": torch.randn(R, C, device=dev).to(torch.bfloat16),
         "do32": torch.randn(R, C, device=dev), "do16": torch.randn(R, C, device=dev).to(torch.bfloat16)}
    for k, dt in (("o32", torch.float32), ("o16", torch.bfloat16), ("da", torch.float32), ("dy", torch.bfloat16)):
        s[k] = torch.empty(R, C, dtype=dt, device=dev)
    s["mean"], s["rstd"] = torch.empty(R, device=dev), torch.empty(R, device=dev)
    s["dg"], s["db"] = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    s["part"] = torch.empty(L.gt_layernorm_bwd_partial_rows(R), 2 * C, device=dev)
    return s


def fwd(s, st):
    _lib.check(L.gt_layernorm_fwd(P(s["a"]), P(s["y"]), C, P(gam), P(beta), P(rm), P(s["o32"]), P(s["o16"]), C, P(s["mean"]), P(s["rstd"]), R, C, EPS,
                                  0.1, 1, 0.0, 0, 0, P(word), st), "fwd")


def head(s):
    return (P(s["a"]), P(s["y"]), C, P(gam), P(beta), P(rm), P(s["mean"]), P(s["rstd"]), R, C, EPS, 0.1, 1, 0.0, 0, 0, P(word),
            P(s["do32"]), P(s["do16"]), C, P(s["da"]), P(s["dy"]), C)


def bwd(s, st):
    _lib.check(L.gt_layernorm_bwd(*head(s), P(s["dg"]), P(s["db"]), st), "bwd")


def partials(s, st):
    _lib.check(L.gt_layernorm_bwd_partials(*head(s), P(s["part"]), st), "partials")


def time_graph(fn, sets):
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        fn(sets[0], _lib.current_stream(dev))                               # one eager launch first
        with torch.cuda.graph(gr, stream=stream):
            for i in range(N):
                fn(sets[i % len(sets)], _lib.current_stream(dev))
    torch.cuda.synchronize()
    for _ in range(3):
        gr.replay()
    out = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            gr.replay()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / (20 * N) * 1e3)
    return out


sets = [make_set() for _ in range(NSETS)]
for s in sets:
    fwd(s, _lib.current_stream(dev))
torch.cuda.synchronize()
name = args[0] if args else "default"
for label, fn in (("gt_layernorm_fwd", fwd), ("gt_layernorm_bwd", bwd), ("gt_layernorm_bwd_partials", partials)):
    for mode, ss in (("warm", sets[:1]), ("rotating", sets)):
        t = time_graph(fn, ss)
        print(f"{name} R={R} C={C} {label} {mode}: " + " ".join(f"{x:.2f}" for x in t) + " us per launch", flush=True)
