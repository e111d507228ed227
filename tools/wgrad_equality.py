"""dev: does a change to the weight-gradient kernels change a result?

    wgrad_equality.py flush [rows] [--lib LIB]   the decoder flush of tools/wgrad_bench.py (120 jobs, 8896 rows by default) and the encoder's 12
                                        k = 3 jobs (min(rows, 3584) rows) in one WgradQueue, seed 0: one sha256 per gradient tensor and one
                                        over all of them.  GT_WGRAD_PAIRED / GT_WGRAD_SLABS choose the form and the slab count as
                                        everywhere; two libraries, or the paired and the 4-wave form, agree if their outputs are equal files.
    wgrad_equality.py cmp A B [C ...]   bench.py --dump-outputs directories, pairwise: max |a - b|, relative to max |b|, elements that differ
"""
import hashlib, itertools, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def flush(args):
    import torch
    from glow_tts_amd import _lib
    if "--lib" in args:
        _lib.LIB_PATH = os.path.abspath(args[args.index("--lib") + 1])
    from glow_tts_amd import flow_impl, wgrad
    from glow_tts_amd.modules import ConvP, WNConvP
    dev, R = torch.device("cuda:0"), int(args[0]) if args and args[0].isdigit() else 8896
    torch.manual_seed(0)
    rows = lambda C, n=R: (torch.randn(n, C, device=dev) * 0.5).to(torch.bfloat16)
    shapes = ([(WNConvP, 192, 384, 5, R)] * 4 + [(WNConvP, 192, 384, 1, R)] * 3 +
              [(WNConvP, 192, 192, 1, R), (WNConvP, 80, 192, 1, R), (ConvP, 192, 160, 1, R)]) * 12
    shapes += [(ConvP, 192, 768, 3, min(R, 3584)), (ConvP, 768, 192, 3, min(R, 3584))] * 6
    convs = []
    for cls, cin, cout, k, n in shapes:
        c = cls(cin, cout, k).to(dev); c.prepare(); convs.append((c, rows(cin, n), rows(cout, n)))
    with wgrad.WgradQueue(dev):
        grads = [flow_impl.conv_param_grads(c, x, dy, x.shape[0]) for c, x, dy in convs]
    torch.cuda.synchronize()
    total = hashlib.sha256()
    for i, ((c, x, _), g) in enumerate(zip(convs, grads)):
        for name, p in c.named_parameters():
            if p in g:
                d = hashlib.sha256(g[p].cpu().numpy().tobytes()).hexdigest()
                total.update(d.encode())
                print(f"job {i:3d} k={c.kernel_size} {c.in_channels:3d}->{c.out_channels:3d} {name:10s} {d}")
    print(f"all: {len(convs)} jobs, {R} rows: {total.hexdigest()}")


def cmp(dirs):
    for a, b in itertools.combinations(dirs, 2):
        parts = []
        for name in ("loss", "mle_loss", "grad_norm", "params", "grads"):
            x, y = np.load(os.path.join(a, name + ".npy")), np.load(os.path.join(b, name + ".npy"))
            d = np.abs(x - y).max()
            parts.append(f"{name} {d:.3e} ({d / max(np.abs(y).max(), 1e-30):.2e} rel, {int((x != y).sum())} differ)")
        print(f"{os.path.basename(a.rstrip('/'))} vs {os.path.basename(b.rstrip('/'))}: " + "; ".join(parts))


if __name__ == "__main__":
    flush(sys.argv[2:]) if sys.argv[1] == "flush" else cmp(sys.argv[2:])
