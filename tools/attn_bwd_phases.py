"""dev: where the T <= 160 attention backward (gt_attn_bwd_fused_kernel) spends its time — shader-clock stamps of the first lane of
every wave of every workgroup (a -DATTN_PHASES=1 build of csrc/attn_mfma.hip made by tools/exp_variant.py), median
over workgroups, in ticks of s_memtime and as a share of the launch.  Shapes of tools/attn_bench.py.

    python tools/exp_variant.py ph attn_mfma -DATTN_PHASES=1
    T=150 python tools/attn_bwd_phases.py glow-tts_amd/build/exp/libglowtts_ph.so"""
import ctypes, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from glow_tts_amd import _lib
_lib.LIB_PATH = os.path.abspath(sys.argv[1])
from glow_tts_amd import ops

dev = torch.device("cuda:0")
L = _lib.lib()
raw = ctypes.CDLL(_lib.LIB_PATH)
B, T, H, D = 32, int(os.environ.get("T", 150)), 2, 96
torch.manual_seed(0)
rc = ops.RowsCtx(torch.randint(T // 2, T + 1, (B,), dtype=torch.int32).to(dev), T)
R, C = rc.R, H * D
q, k, v, do = [torch.randn(R, C, device=dev).to(torch.bfloat16) for _ in range(4)]
Ek = torch.randn(9, D, device=dev) * 0.1; Ev = torch.randn(9, D, device=dev) * 0.1
o = torch.zeros(R, C, dtype=torch.bfloat16, device=dev); P = torch.empty(B, H, T, T, device=dev)
wsb = L.gt_attn_bwd_workspace_bytes(B, T, H); ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
dq, dk, dv = [torch.zeros(R, C, dtype=torch.bfloat16, device=dev) for _ in range(3)]
dEk = torch.zeros_like(Ek); dEv = torch.zeros_like(Ev)
st = _lib.current_stream(dev)
assert L.gt_attn_fwd(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), C, _lib.ptr(Ek), _lib.ptr(Ev), _lib.ptr(rc.lengths), _lib.ptr(o), C, _lib.ptr(P),
                     B, T, rc.Tp, None, H, D, 4, 0.1, 7, None, st) == 0
for _ in range(3):
    assert L.gt_attn_bwd(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), C, _lib.ptr(Ek), _lib.ptr(Ev), _lib.ptr(rc.lengths), _lib.ptr(do), C, _lib.ptr(P), _lib.ptr(ws), wsb,
                         _lib.ptr(dq), _lib.ptr(dk), _lib.ptr(dv), C, _lib.ptr(dEk), _lib.ptr(dEv), B, T, rc.Tp, None, H, D, 4, 0.1, 7, None, st) == 0
torch.cuda.synchronize()
buf = np.zeros(8 * 128 * 16, dtype=np.uint64)
assert raw.gt_dev_attn_phases(buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(buf.nbytes)) == 0
NAMES = os.environ.get("ATTN_PHASE_NAMES")            # "half:idx=name;..." for another stamped build of the same buffer layout
if NAMES:
    sets = {}
    for item in NAMES.split(";"):
        key, nm = item.split("=", 1)
        hf, idx = key.split(":")
        sets.setdefault(int(hf), []).append((int(idx), nm))
    nwg = int(os.environ.get("ATTN_PHASE_WGS", 128))
else:
    names = [(1, "stage K, V, Ev, EkT, zero band tables, barrier"), (2, "dO fragments, DOE = Ev dO^T (6 MFMA)"),
             (3, "pass A: 5 x (dPd^T 6 MFMA, P loads, hash, Dsum)"), (4, "pass B: 5 x (dPd^T, P loads, dS^T/P'^T -> LDS, P'^T rows out, dQ^T 6 MFMA)"),
             (5, "Ek band MFMA, dq stores issued"), (6, "fence + barrier (waits for the slowest query tile)"),
             (7, "stage Q, dO, zero dE tables, barrier"), (9, "key tile: P'^T row loads, dK^T, dV^T (60 MFMA), stores issued"),
             (10, "waves 5..7: dEk / dEv contraction of query tiles {0, 3}, {1, 4}, {2}"),
             (11, "dS^T rows LDS -> workspace, barrier, global atomics, end")]
    tile = [n for n in names if n[0] not in (10,)]
    rest = [n for n in names if n[0] in (1, 6, 7, 10, 11)]
    sets, nwg = {w: (tile if w < 5 else rest) for w in range(8)}, B * H
for hf, names in sorted(sets.items()):
    ph = buf.reshape(8, 128, 16)[hf, :nwg].astype(np.int64)
    t = ph[:, [i for i, _ in names]] - ph[:, [0]]
    med = np.median(t, axis=0)
    total = med[-1]
    print(f"-- T={T} wave {hf}: {nwg} workgroups, launch = {total:.0f} cycles (median); start skew p5..p95 = "
          f"{np.percentile(ph[:, 0] - ph[:, 0].min(), [5, 95])}")
    prev = 0.0
    for (i, nm), m in zip(names, med):
        print(f"   {nm:84s} {m - prev:8.0f}  ({(m - prev) / total * 100:5.1f} %)   at {m:8.0f}")
        prev = m
