"""Micro-benchmark of gt_attn_fwd / gt_attn_bwd (dev tool).  T=<tokens> DROP=<p, default 0.1> python tools/attn_bench.py [--no-p | --stats | --stats-only]
--no-p: the forward alone, with P and with P == NULL (long shapes only), and the bytes each call writes, computed from the shapes
(out: B T H D bf16; P: B H T^2 fp32), over its time.
--stats: forward and backward of both forms in one process (long shapes only): the saved-P pair and gt_attn_fwd_stats /
gt_attn_bwd_stats, with the bytes each form allocates between forward and backward and for the backward's workspace.
--stats-only: the stats pair alone; P and the T^2 workspace are never allocated (B = 32 at T = 4096: 4.3 GB each)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from glow_tts_amd import _lib, ops
dev = torch.device("cuda:0")
L = _lib.lib()
B, T, H, D = int(os.environ.get("B", 32)), int(os.environ.get("T", 150)), 2, 96
DROP = float(os.environ.get("DROP", 0.1))
STATS_ONLY = "--stats-only" in sys.argv
STATS = STATS_ONLY or "--stats" in sys.argv
rc = ops.RowsCtx(torch.randint(T // 2, T + 1, (B,), dtype=torch.int32).to(dev), T)
R, C = rc.R, H * D
q, k, v, do = [torch.randn(R, C, device=dev).to(torch.bfloat16) for _ in range(4)]
Ek = torch.randn(9, D, device=dev) * 0.1; Ev = torch.randn(9, D, device=dev) * 0.1
o = torch.zeros(R, C, dtype=torch.bfloat16, device=dev)
dq, dk, dv = [torch.zeros(R, C, dtype=torch.bfloat16, device=dev) for _ in range(3)]
dEk = torch.zeros_like(Ek); dEv = torch.zeros_like(Ev)
st = _lib.current_stream(dev)
if not STATS_ONLY:
    P = torch.empty(B, H, T, T, device=dev)
    wsb = L.gt_attn_bwd_workspace_bytes(B, T, H); dS = torch.empty(wsb, dtype=torch.uint8, device=dev)
if STATS:
    sb, swb = L.gt_attn_stats_bytes(B, T, H), L.gt_attn_bwd_stats_workspace_bytes(B, T, H)
    stats = torch.empty(sb, dtype=torch.uint8, device=dev); sws = torch.empty(swb, dtype=torch.uint8, device=dev)
def fwd(P=None if STATS_ONLY else P):
    assert L.gt_attn_fwd(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), C, _lib.ptr(Ek), _lib.ptr(Ev), _lib.ptr(rc.lengths), _lib.ptr(o), C, _lib.ptr(P),
                         B, T, rc.Tp, None, H, D, 4, DROP, 7, None, st) == 0
def bwd():
    assert L.gt_attn_bwd(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), C, _lib.ptr(Ek), _lib.ptr(Ev), _lib.ptr(rc.lengths), _lib.ptr(do), C, _lib.ptr(P), _lib.ptr(dS), wsb,
                         _lib.ptr(dq), _lib.ptr(dk), _lib.ptr(dv), C, _lib.ptr(dEk), _lib.ptr(dEv), B, T, rc.Tp, None, H, D, 4, DROP, 7, None, st) == 0
def fwd_stats():
    assert L.gt_attn_fwd_stats(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), C, _lib.ptr(Ek), _lib.ptr(Ev), _lib.ptr(rc.lengths), _lib.ptr(o), C, _lib.ptr(stats),
                               B, T, rc.Tp, None, H, D, 4, DROP, 7, None, st) == 0
def bwd_stats():
    assert L.gt_attn_bwd_stats(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), C, _lib.ptr(Ek), _lib.ptr(Ev), _lib.ptr(rc.lengths), _lib.ptr(do), C, _lib.ptr(stats), _lib.ptr(sws), swb,
                               _lib.ptr(dq), _lib.ptr(dk), _lib.ptr(dv), C, _lib.ptr(dEk), _lib.ptr(dEv), B, T, rc.Tp, None, H, D, 4, DROP, 7, None, st) == 0
def timeit(fn, n=30):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3
if STATS:
    n = 10 if T > 2048 else 30
    line = f"T={T} B={B} p={DROP}"
    if not STATS_ONLY:
        t_f, t_b = timeit(fwd, n), timeit(bwd, n)
        line += f"  saved P: fwd {t_f:.1f} us  bwd {t_b:.1f} us  (P {4 * B * H * T * T / 1e6:.1f} MB kept, workspace {wsb / 1e6:.1f} MB)"
    t_fs, t_bs = timeit(fwd_stats, n), timeit(bwd_stats, n)
    line += f"  stats: fwd {t_fs:.1f} us  bwd {t_bs:.1f} us  (stats {sb / 1e6:.2f} MB kept, workspace {swb / 1e6:.2f} MB)"
    if not STATS_ONLY:
        line += f"  stats / saved P: fwd {t_fs / t_f:.2f}  bwd {t_bs / t_b:.2f}"
    print(line, flush=True)
elif "--no-p" in sys.argv:
    t_p, t_n = timeit(fwd), timeit(lambda: fwd(None))
    b_o, b_p = B * T * C * 2, 4 * B * H * T * T
    print(f"T={T} p={DROP} fwd with P {t_p:.1f} us ({(b_o + b_p) / 1e6:.1f} MB written, {(b_o + b_p) / t_p / 1e6:.2f} TB/s)  "
          f"fwd P=NULL {t_n:.1f} us ({b_o / 1e6:.1f} MB written, {b_o / t_n / 1e6:.3f} TB/s)", flush=True)
else:
    print(f"T={T} fwd {timeit(fwd):.1f} us  bwd {timeit(bwd):.1f} us", flush=True)
