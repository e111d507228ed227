"""dev: does a change to csrc/align_loss.hip change a result?

    align_loss_equality.py [--lib LIB]

Every entry of the file once per case on fixed seeded operands, one sha256 per output tensor: two libraries agree if their outputs
are equal files (profiles/align_loss_share_*.txt: the parent's against the shared helpers').  The fused-equals-unfused tests cannot
see both chains drifting together; this can.  Cases: B = 3, C in {6, 80}, (T_x, T_y) in SHAPES, with and without x_logs — the unfused
chain and the fused one with and without the duration term, each backward with gscale 1.0 and 0.37; gt_prior_expand_bwd at
(513, 640), the first token count of its dynamic-LDS form; gt_logp_f32 once per mean_only branch; gt_length_mask for both length
types.  No launch is repeated or retried: run it under the caller's timeout.
"""
import hashlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

B, CS, SHAPES, GSCALES = 3, [6, 80], [(1, 4), (7, 32), (70, 96), (150, 160)], [1.0, 0.37]
F32 = torch.float32


def monotone_map(rng, n_tok, n_frames, Ty):
    """frame2token of one utterance: n_tok durations (zeros allowed, one of 67 frames where there is room) that sum to n_frames,
    -1 on the padded frames"""
    d = np.zeros(n_tok, dtype=np.int64)
    rest = n_frames
    if n_frames >= 70 and n_tok >= 2:
        d[1], rest = 67, rest - 67
    cuts = np.sort(rng.integers(0, rest + 1, size=n_tok - 1))
    d += np.diff(np.concatenate([[0], cuts, [rest]]))
    f2t = -np.ones(Ty, dtype=np.int32)
    f2t[:n_frames] = np.repeat(np.arange(n_tok), d)
    return d, f2t


def operands(C, Tx, Ty, dev):
    rng = np.random.default_rng(1000 * C + 10 * Tx + Ty)
    g = torch.Generator().manual_seed(7 * C + Tx + Ty)
    x_len, y_len = [Tx, 1, min(Tx, 2)], [Ty, max(1, Ty - 3), min(Ty, 2)]
    dur, f2t = np.zeros((B, Tx), dtype=np.int64), np.zeros((B, Ty), dtype=np.int32)
    for b in range(B):
        dur[b, :x_len[b]], f2t[b] = monotone_map(rng, x_len[b], y_len[b], Ty)
    on = torch.arange(Tx)[None, :] < torch.tensor(x_len)[:, None]
    d = dict(z=torch.randn(B, C, Ty, generator=g) * 1.5, x_m=torch.randn(B, C, Tx, generator=g),
             x_logs=(torch.randn(B, C, Tx, generator=g) * 0.7).clamp_(-2, 2), f2t=torch.from_numpy(f2t),
             logw=torch.randn(B, Tx, generator=g) * on, w=torch.from_numpy(dur).float(), x_len=torch.tensor(x_len, dtype=torch.int32),
             logdet=torch.randn(B, generator=g) * 50, mask=(torch.arange(Ty)[None, :] < torch.tensor(y_len)[:, None]).float()[:, None, :])
    return {k: v.to(dev) for k, v in d.items()}


def main(args):
    from glow_tts_amd import _lib
    if "--lib" in args:
        _lib.LIB_PATH = os.path.abspath(args[args.index("--lib") + 1])
    dev = torch.device("cuda:0")
    call, st = _lib.call, _lib.current_stream(dev)
    new = lambda *s: torch.full(s, float("nan"), dtype=F32, device=dev)       # noqa: E731  (an element left unwritten shows in the hash)
    total, count = hashlib.sha256(), [0]

    def show(tag, **tensors):
        torch.cuda.synchronize()
        for name, t in tensors.items():
            if t is not None:
                h = hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()
                total.update(h.encode())
                count[0] += 1
                print(f"{tag:58s} {name:10s} {h}")

    for C in CS:
        for Tx, Ty in SHAPES:
            d, n = operands(C, Tx, Ty, dev), B * C * Ty
            for logs in (False, True):
                tag = f"C={C} {Tx}x{Ty} x_logs={'set' if logs else 'NULL'}"
                x_logs = d["x_logs"] if logs else None
                # the unfused chain
                z_m, z_logs = new(B, C, Ty), (new(B, C, Ty) if logs else None)
                call.gt_prior_expand(d["x_m"], d["f2t"], z_m, B, C, Tx, Ty, st)
                if logs:
                    call.gt_prior_expand(x_logs, d["f2t"], z_logs, B, C, Tx, Ty, st)
                acc, out2, l_length = new(2 * _lib.MLE_PARTS), new(2), new(B)
                call.gt_mle_sums(d["z"], z_m, z_logs, acc, n, st)
                call.gt_mle_finish(acc, d["logdet"], d["mask"], d["mask"].numel(), B, C, out2, st)
                call.gt_duration_loss_fwd(d["logw"], d["w"], d["x_len"], B, Tx, l_length, st)
                show(tag + " unfused", z_m=z_m, z_logs=z_logs, acc=acc, out2=out2, l_length=l_length)
                for gscale in GSCALES:
                    gs = torch.tensor([gscale], dtype=F32, device=dev)
                    dz, dm, dlogs, dlogdet = new(B, C, Ty), new(B, C, Ty), (new(B, C, Ty) if logs else None), new(B)
                    call.gt_mle_bwd(d["z"], z_m, z_logs, gs, dz, dm, dlogs, n, out2[1:].data_ptr(), dlogdet, B, st)
                    dx_m, dx_logs, dlogw = new(B, C, Tx), (new(B, C, Tx) if logs else None), new(B, Tx)
                    call.gt_prior_expand_bwd(dm, d["f2t"], dx_m, B, C, Tx, Ty, st)
                    if logs:
                        call.gt_prior_expand_bwd(dlogs, d["f2t"], dx_logs, B, C, Tx, Ty, st)
                    call.gt_duration_loss_bwd(d["logw"], d["w"], d["x_len"], gs.expand(B).contiguous(), B, Tx, dlogw, st)
                    show(f"{tag} unfused gscale={gscale}", dz=dz, dm=dm, dlogs=dlogs, dlogdet=dlogdet, dx_m=dx_m, dx_logs=dx_logs, dlogw=dlogw)
                # the chain in three launches
                for dur in (True, False):
                    ftag = f"{tag} fused duration={'on' if dur else 'off'}"
                    logw, w, x_len = (d["logw"], d["w"], d["x_len"]) if dur else (None, None, None)
                    f_zm, f_zl, f_acc = new(B, C, Ty), (new(B, C, Ty) if logs else None), new(2 * _lib.MLE_PARTS)
                    f_ll, out4 = (new(B) if dur else None), new(4)
                    call.gt_align_loss_fwd(d["z"], d["x_m"], x_logs, d["f2t"], logw, w, x_len, f_zm, f_zl, f_acc, f_ll, B, C, Tx, Ty, st)
                    call.gt_align_loss_finish(f_acc, d["logdet"], d["mask"], d["mask"].numel(), f_ll, B, C, out4, st)
                    show(ftag, z_m=f_zm, z_logs=f_zl, acc=f_acc, l_length=f_ll, out4=out4)
                    for gscale in GSCALES:
                        gs = torch.tensor([gscale], dtype=F32, device=dev)
                        dz, dx_m, dx_logs = new(B, C, Ty), new(B, C, Tx), (new(B, C, Tx) if logs else None)
                        dlogdet, dlogw = new(B), (new(B, Tx) if dur else None)
                        call.gt_align_loss_bwd(d["z"], f_zm, f_zl, d["f2t"], logw, w, x_len, gs, out4[1:].data_ptr(), dz, dx_m, dx_logs,
                                               dlogdet, dlogw, B, C, Tx, Ty, st)
                        show(f"{ftag} gscale={gscale}", dz=dz, dx_m=dx_m, dx_logs=dx_logs, dlogdet=dlogdet, dlogw=dlogw)

    # gt_prior_expand_bwd past acc[4][512]
    Bp, Cp, Tx, Ty = 2, 3, 513, 640
    rng, g = np.random.default_rng(513), torch.Generator().manual_seed(513)
    f2t = torch.from_numpy(np.stack([monotone_map(rng, Tx, Ty - 17 * b, Ty)[1] for b in range(Bp)])).to(dev)
    dzm, dxm = torch.randn(Bp, Cp, Ty, generator=g).to(dev), new(Bp, Cp, Tx)
    call.gt_prior_expand_bwd(dzm, f2t, dxm, Bp, Cp, Tx, Ty, st)
    show(f"gt_prior_expand_bwd B={Bp} C={Cp} {Tx}x{Ty}", dx_m=dxm)

    # gt_logp_f32: mean_only (x_logs NULL) and not; gt_length_mask: int32 and int64 lengths
    Bl, Cl, Tx, Ty = 2, 6, 40, 70
    g = torch.Generator().manual_seed(40)
    x_m, x_logs, z = (torch.randn(Bl, Cl, t, generator=g).to(dev) for t in (Tx, Tx, Ty))
    for name, s in (("NULL", None), ("set", x_logs * 0.5)):
        logp = new(Bl, Tx, Ty)
        call.gt_logp_f32(x_m, s, z, logp, Bl, Cl, Tx, Ty, st)
        show(f"gt_logp_f32 B={Bl} C={Cl} {Tx}x{Ty} x_logs={name}", logp=logp)
    for dt in (torch.int32, torch.int64):
        lens, mask = torch.tensor([67, 1, 30], dtype=dt, device=dev), new(3, 67)
        call.gt_length_mask(lens, int(dt == torch.int64), mask, 3, 67, st)
        show(f"gt_length_mask 3x67 {str(dt).split('.')[1]}", mask=mask)
    print(f"all: {count[0]} tensors: {total.hexdigest()}")


if __name__ == "__main__":
    main(sys.argv[1:])
