"""dev: do the paired weight-gradient launches change a result?

    wgrad_equality.py flush             the decoder flush of tools/wgrad_bench.py (120 jobs, 8896 rows, seed 0) through the paired form and
                                        through the 4-wave form (wgrad.PAIRED = False) on identical inputs: sha256 of every gradient tensor
    wgrad_equality.py cmp A B [C ...]   bench.py --dump-outputs directories, pairwise: max |a - b|, relative to max |b|, elements that differ
"""
import hashlib, itertools, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def flush():
    import torch
    from glow_tts_amd import flow_impl, wgrad
    from glow_tts_amd.modules import ConvP, WNConvP
    dev, R = torch.device("cuda:0"), 8896
    torch.manual_seed(0)
    rows = lambda C: (torch.randn(R, C, device=dev) * 0.5).to(torch.bfloat16)
    convs = []
    for blk in range(12):
        shapes = [(WNConvP, 192, 384, 5)] * 4 + [(WNConvP, 192, 384, 1)] * 3 + [(WNConvP, 192, 192, 1), (WNConvP, 80, 192, 1), (ConvP, 192, 160, 1)]
        for cls, cin, cout, k in shapes:
            c = cls(cin, cout, k).to(dev); c.prepare(); convs.append((c, rows(cin), rows(cout)))
    out = {}
    for paired in (True, False):
        wgrad.PAIRED = paired
        with wgrad.WgradQueue(dev):
            grads = [flow_impl.conv_param_grads(c, x, dy, R) for c, x, dy in convs]
        torch.cuda.synchronize()
        out[paired] = [{name: hashlib.sha256(g[p].cpu().numpy().tobytes()).hexdigest() for name, p in c.named_parameters() if p in g}
                       for (c, _, _), g in zip(convs, grads)]
    for name in sorted({n for d in out[True] for n in d}):
        pairs = [(a[name], b[name]) for a, b in zip(out[True], out[False]) if name in a]
        print(f"flush {name:10s}: {sum(a == b for a, b in pairs)} of {len(pairs)} tensors bit-identical to the 4-wave form's")


def cmp(dirs):
    for a, b in itertools.combinations(dirs, 2):
        parts = []
        for name in ("loss", "mle_loss", "grad_norm", "params", "grads"):
            x, y = np.load(os.path.join(a, name + ".npy")), np.load(os.path.join(b, name + ".npy"))
            d = np.abs(x - y).max()
            parts.append(f"{name} {d:.3e} ({d / max(np.abs(y).max(), 1e-30):.2e} rel, {int((x != y).sum())} differ)")
        print(f"{os.path.basename(a.rstrip('/'))} vs {os.path.basename(b.rstrip('/'))}: " + "; ".join(parts))


if __name__ == "__main__":
    flush() if sys.argv[1] == "flush" else cmp(sys.argv[2:])
