"""Timing of the long-lattice MAS kernel (gt_mas_long_f32) on the GPU (dev tool, not the bench contract).

    python tools/mas_long_timing.py [> profiles/mas_long_timing.txt]

Device events, 5 warm-up and 50 timed calls per shape, lengths drawn as tests/test_mas_gpu.py::test_full_size_properties draws
them.  (1) against the host: the same lattice, already in host memory, through the reference's Cython core (oracle/_ref, serial
as the reference builds it) and through the C restatement with one utterance per OpenMP thread at 16 threads, best of 3 each —
the device-to-host copy the reference also pays is left out, which favours the host.  (2) against gt_mas_f32 on a lattice both
kernels take, the two entries alternating in one process: what keeping the direction words in HBM costs.
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from glow_tts_amd import _lib  # noqa: E402
from oracle import mas as omas  # noqa: E402

dev = torch.device("cuda:0")
L = _lib.lib()
WARM, N = 5, 50


def lattice(B, T_x, T_y, seed):
    g = torch.Generator().manual_seed(seed)
    t_x = torch.randint(max(1, T_x // 3), T_x + 1, (B,), generator=g, dtype=torch.int32)
    t_y = (torch.randint(T_y // 4, T_y // 2 + 1, (B,), generator=g, dtype=torch.int32) * 2)
    t_y = torch.maximum(t_y, t_x + (t_x % 2))
    t_x[0], t_y[0] = T_x, T_y
    v = (torch.randn(B, T_x, T_y, generator=g) * 5 - 100)
    return v, t_x, t_y


class Entry:
    def __init__(self, name, v, t_x, t_y):
        self.name = name
        self.B, self.T_x, self.T_y = v.shape
        self.v, self.t_x, self.t_y = v.to(dev), t_x.to(dev), t_y.to(dev)
        self.path = torch.empty_like(self.v)
        nbytes = (L.gt_mas_workspace_bytes if name == "gt_mas_f32" else L.gt_mas_long_workspace_bytes)(self.B, self.T_x, self.T_y)
        self.nbytes, self.ws = nbytes, torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def run(self):
        rc = getattr(L, self.name)(_lib.ptr(self.v), None, _lib.ptr(self.t_x), _lib.ptr(self.t_y), _lib.ptr(self.path), _lib.GT_DT_F32,
                                   None, None, self.B, self.T_x, self.T_y, self.v.stride(0), self.v.stride(1), _lib.ptr(self.ws),
                                   self.nbytes, None, _lib.current_stream(dev))
        assert rc == 0, (self.name, rc)

    def time_ms(self, n=N):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            self.run()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n


def best_of(fn, value, n=3):
    best = None
    for _ in range(n):
        v = np.ascontiguousarray(value.copy()); p = np.zeros(v.shape, dtype=np.int32)
        t0 = time.perf_counter()
        fn(p, v)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, p


print(f"# {L.gt_version().decode()}; {WARM} warm-up + {N} timed calls, device events; host: best of 3, lattice in host memory")
print("# (1) gt_mas_long_f32 against the host")
for (B, T_x, T_y) in [(16, 384, 1304), (16, 600, 1400), (8, 1024, 4096)]:
    assert T_x > 512 or L.gt_mas_lds_bytes(T_x, T_y) > 160 * 1024
    v, t_x, t_y = lattice(B, T_x, T_y, 1234)
    e = Entry("gt_mas_long_f32", v, t_x, t_y)
    for _ in range(WARM):
        e.run()
    torch.cuda.synchronize()
    ms = e.time_ms()
    got = e.path.cpu().numpy().astype(np.int32)
    txn, tyn = t_x.numpy(), t_y.numpy()
    omp, p = best_of(lambda p, v: omas.oracle_maximum_path_omp(p, v, txn, tyn, 16), v.numpy())
    assert np.array_equal(p, got), "device path != host path"
    line = (f"B={B} T_x={T_x} T_y={T_y}: GPU {ms * 1e3:8.1f} us/batch {B / ms * 1e3:9.0f} align/s | C port, 16 OpenMP threads "
            f"{omp * 1e6:9.1f} us/batch {B / omp:8.0f} align/s, GPU {omp * 1e3 / ms:5.2f}x")
    if omas.ref_module() is not None:
        ref, p = best_of(lambda p, v: omas.ref_maximum_path_c(p, v, txn, tyn), v.numpy())
        assert np.array_equal(p, got), "device path != reference path"
        line += f" | reference core.pyx (serial) {ref * 1e6:9.1f} us/batch {B / ref:7.0f} align/s, GPU {ref * 1e3 / ms:6.2f}x"
    print(line, flush=True)

print("# (2) gt_mas_long_f32 forced where gt_mas_f32 runs (alternating in one process)")
v, t_x, t_y = lattice(32, 375, 872, 1235)
a, b = Entry("gt_mas_f32", v, t_x, t_y), Entry("gt_mas_long_f32", v, t_x, t_y)
for _ in range(WARM):
    a.run(); b.run()
torch.cuda.synchronize()
ta, tb = [], []
for _ in range(5):
    ta.append(a.time_ms(10)); tb.append(b.time_ms(10))
assert torch.equal(a.path, b.path)
print(f"B=32 T_x=375 T_y=872: gt_mas_f32 {np.median(ta) * 1e3:.1f} us/batch (min {min(ta) * 1e3:.1f}, max {max(ta) * 1e3:.1f}) | "
      f"gt_mas_long_f32 {np.median(tb) * 1e3:.1f} us/batch (min {min(tb) * 1e3:.1f}, max {max(tb) * 1e3:.1f}) | "
      f"ratio {np.median(tb) / np.median(ta):.2f}")
