"""dev: does a change to the MFMA attention kernels (csrc/attn_mfma.hip, csrc/attn_long.hip, csrc/attn_frag.h) change a bit of what
they return?

    attn_trace.py > trace.txt                 one line per case and tensor: a sha256 of the tensor's bytes
    attn_trace.py --save DIR                  also writes dEk / dEv of every backward to DIR/<case>.pt
    attn_trace.py --against DIR               also prints, per case, the largest |dEk - saved| and |dEv - saved| ("# dE" lines)

Two trees agree if their listings without the "#" lines are equal files (profiles/attn_parts_trace_{parent,new}.txt;
tests/test_attn_trace_gpu.py compares a fresh run with the parent's).  Entries per case: gt_attn_fwd with P; gt_attn_fwd with
P == NULL, gt_attn_fwd_stats and gt_attn_bwd_stats (key-tiled shapes only); gt_attn_bwd.  Every buffer starts zero-filled and is
hashed whole: out, P, stats, the dS^T | P'^T workspace, the record workspace of the stats backward, dq, dk, dv — each element has one
writing lane, so the bits are deterministic.  dEk and dEv are fp32 atomic sums over waves and workgroups: their bits depend on the
arrival order and are not hashed; compare them (--save / --against) with a second run of the same tree as the yardstick.

Cases: H = 2, D = 96, window 4, lens [max(T - 7, 1), 1, T]; each T once ragged with p = 0.1 and the seed word on the device, once
uniform with p = 0 and non-zero dout on padded rows.  T per path, the smallest at which its edges occur:
  one workgroup per utterance-head (T <= 160)  3 (one partial tile), 33 (a tile plus one key), 160 (the full five)
  8 tiles                                      161, 256
  12 tiles                                     257, 384
  key-tiled                                    506 (scalar P path, partial last tile), 513 (one key past a tile: a workgroup of
                                               staging-only waves)
No launch is repeated or retried: run it under the caller's timeout."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

H, D, WIN, B = 2, 96, 4, 3
SEED, WORD = 0x51ED270B, 0x1234ABCD
TS = (3, 33, 160, 161, 256, 257, 384, 506, 513)
CASES = [(T, ragged) for T in TS for ragged in (True, False)]


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def run_case(T, ragged):
    """-> (case name, [(tensor name, sha256)], {name: dEk / dEv tensors on the host})"""
    from glow_tts_amd import _lib, ops
    L = _lib.lib()
    dev = torch.device("cuda:0")
    C = H * D
    p = 0.1 if ragged else 0.0
    name = f"T={T} {'ragged p=0.1 word' if ragged else 'uniform p=0 dirty'}"
    lens = [max(T - 7, 1), 1, T]
    lens_t = torch.tensor(lens, dtype=torch.int32, device=dev)
    rc = ops.RowsCtx(lens_t, T, lengths_host=lens, round_to=128) if ragged else ops.RowsCtx(lens_t, T)
    R = rc.R
    g = torch.Generator().manual_seed(7 * T + D + int(ragged))
    m = rc.rowmask[:, None].cpu()
    qkv = ((torch.randn(R, 3 * C, generator=g) * 0.5) * m).to(torch.bfloat16).to(dev)
    do = torch.randn(R, C, generator=g) * m
    Ek, Ev = (torch.randn(2 * WIN + 1, D, generator=g) * 0.1).to(dev), (torch.randn(2 * WIN + 1, D, generator=g) * 0.1).to(dev)
    if not ragged:                                                    # padded frames only: halo rows stay zero (the rows contract)
        for b in range(B):
            r0 = b * rc.Tp + ops.HALO
            do[r0 + lens[b]:r0 + T] = torch.randn(T - lens[b], C, generator=g)
    do = do.to(torch.bfloat16).to(dev)
    wd = torch.tensor([WORD], dtype=torch.int32, device=dev) if ragged else None
    st, r0p = _lib.current_stream(dev), _lib.ptr(rc.row0)
    q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    long_shape = bool(L.gt_attn_long_shape(T, D, WIN))

    def zeros(*shape, dtype=torch.float32):
        return torch.zeros(*shape, dtype=dtype, device=dev)

    def fwd(P, out):
        _lib.check(L.gt_attn_fwd(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), 3 * C, _lib.ptr(Ek), _lib.ptr(Ev), _lib.ptr(rc.lengths), _lib.ptr(out), C,
                                 _lib.ptr(P), B, T, rc.Tp, r0p, H, D, WIN, p, SEED, _lib.ptr(wd), st), "gt_attn_fwd")

    lines, dE = [], {}
    out, P = zeros(R, C, dtype=torch.bfloat16), zeros(B, H, T, T)
    fwd(P, out)
    lines += [("fwd out", sha(out)), ("fwd P", sha(P))]
    wsb = L.gt_attn_bwd_workspace_bytes(B, T, H)
    ws, grads = zeros(wsb, dtype=torch.uint8), zeros(R, 3 * C, dtype=torch.bfloat16)
    dEk, dEv = zeros(2 * WIN + 1, D), zeros(2 * WIN + 1, D)
    _lib.check(L.gt_attn_bwd(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), 3 * C, _lib.ptr(Ek), _lib.ptr(Ev), _lib.ptr(rc.lengths), _lib.ptr(do), C,
                             _lib.ptr(P), _lib.ptr(ws), wsb, _lib.ptr(grads[:, :C]), _lib.ptr(grads[:, C:2 * C]), _lib.ptr(grads[:, 2 * C:]), 3 * C,
                             _lib.ptr(dEk), _lib.ptr(dEv), B, T, rc.Tp, r0p, H, D, WIN, p, SEED, _lib.ptr(wd), st), "gt_attn_bwd")
    lines += [("bwd workspace", sha(ws)), ("bwd dq", sha(grads[:, :C])), ("bwd dk", sha(grads[:, C:2 * C])), ("bwd dv", sha(grads[:, 2 * C:]))]
    dE["bwd dEk"], dE["bwd dEv"] = dEk.cpu(), dEv.cpu()
    if long_shape:
        out2 = zeros(R, C, dtype=torch.bfloat16)
        fwd(None, out2)
        lines.append(("fwd P=NULL out", sha(out2)))
        out3, stats = zeros(R, C, dtype=torch.bfloat16), zeros(L.gt_attn_stats_bytes(B, T, H), dtype=torch.uint8)
        _lib.check(L.gt_attn_fwd_stats(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), 3 * C, _lib.ptr(Ek), _lib.ptr(Ev), _lib.ptr(rc.lengths), _lib.ptr(out3), C,
                                       _lib.ptr(stats), B, T, rc.Tp, r0p, H, D, WIN, p, SEED, _lib.ptr(wd), st), "gt_attn_fwd_stats")
        lines += [("fwd_stats out", sha(out3)), ("fwd_stats stats", sha(stats))]
        swb = L.gt_attn_bwd_stats_workspace_bytes(B, T, H)
        sws, grads2 = zeros(swb, dtype=torch.uint8), zeros(R, 3 * C, dtype=torch.bfloat16)
        dEk2, dEv2 = zeros(2 * WIN + 1, D), zeros(2 * WIN + 1, D)
        _lib.check(L.gt_attn_bwd_stats(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), 3 * C, _lib.ptr(Ek), _lib.ptr(Ev), _lib.ptr(rc.lengths), _lib.ptr(do), C,
                                       _lib.ptr(stats), _lib.ptr(sws), swb, _lib.ptr(grads2[:, :C]), _lib.ptr(grads2[:, C:2 * C]),
                                       _lib.ptr(grads2[:, 2 * C:]), 3 * C, _lib.ptr(dEk2), _lib.ptr(dEv2), B, T, rc.Tp, r0p, H, D, WIN, p, SEED,
                                       _lib.ptr(wd), st), "gt_attn_bwd_stats")
        lines += [("bwd_stats workspace", sha(sws)), ("bwd_stats dq", sha(grads2[:, :C])), ("bwd_stats dk", sha(grads2[:, C:2 * C])),
                  ("bwd_stats dv", sha(grads2[:, 2 * C:]))]
        dE["bwd_stats dEk"], dE["bwd_stats dEv"] = dEk2.cpu(), dEv2.cpu()
    torch.cuda.synchronize()
    return name, lines, dE


def listing():
    """[(line of the listing, case name, dE tensors)]: the text tests/test_attn_trace_gpu.py compares"""
    out = []
    for T, ragged in CASES:
        name, lines, dE = run_case(T, ragged)
        out.append(([f"{name} | {what} {digest}" for what, digest in lines], name, dE))
    return out


def main(argv):
    save = argv[argv.index("--save") + 1] if "--save" in argv else None
    against = argv[argv.index("--against") + 1] if "--against" in argv else None
    if save:
        os.makedirs(save, exist_ok=True)
    for lines, name, dE in listing():
        print("\n".join(lines), flush=True)
        fname = name.replace(" ", "_").replace("=", "") + ".pt"
        if save:
            torch.save(dE, os.path.join(save, fname))
        if against:
            ref = torch.load(os.path.join(against, fname))
            print(f"# dE {name} | " + "  ".join(f"max|{n} - saved| {float((t - ref[n]).abs().max()):.3e}" for n, t in dE.items()), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
