"""dev: does a change to the between-WaveNet kernels (csrc/wn_boundary.hip), the five-launch flow kernels (csrc/flow_ops.hip) or the
row maths they share (csrc/flow_rows.h) change a bit of what they return?

    wn_boundary_trace.py > trace.txt          one line per pass, launch and tensor: a sha256 of the tensor's bytes
    wn_boundary_trace.py --save DIR           also writes the atomic sums of every pass to DIR/<pass>.pt
    wn_boundary_trace.py --against DIR        also prints, per pass and sum, the largest |sum - saved| ("# sum" lines)
    wn_boundary_trace.py --against DIR --yardstick DIR2    DIR2: a second --save of the tree that wrote DIR; each "# sum" line then also
                                              carries max|saved2 - saved| and OVER where |sum - saved| is more than twice that

Two trees agree if their listings without the "#" lines are equal files (profiles/wn_boundary_parts_trace_{parent,new}.txt;
tests/test_wn_boundary_trace_gpu.py compares a fresh run with the parent's).  A pass is the 3-block decoder of
tests/test_wn_boundary_fp64_gpu.py on one of its three layouts (the smallest shapes at which the tile edge, the segmented scan and the
second trip of the per-utterance loops occur), sigmoid_scale off and on: train forward + backward and eval reverse are recorded with
flow_impl.BOUNDARY_TRACE (the ragged layouts with the folded squeeze / unsqueeze forms, the uniform one on rows), and every launch is
issued once more on pre-filled buffers: row outputs on a canary, [B, 80, T] outputs on zeros, accumulators on a non-zero prior,
pg_partial on NaN.  Its row operands (acts, y, z, dh, dx_in, x, logs_raw, ..) are redrawn from a seed of their own, masked: the recorded
ones come out of the WaveNet kernels, whose dropout masks follow the process's step state, and a listing must not depend on what ran
before it in the process.  Every backward head runs on both parameter-gradient routes.  Hashed: the tensors with one writer per element —
wn_out, logs_raw, z, y_next, y0_bf16, h_next, z_bct; dx_out, dout, dwn_out, via_skip, dx_bct, pg_partial; x, h_next, x_bct — and, for
the six five-launch kernels called on the operands of the recorded launch fwd[1], z, x, dx, dout_bf16, y, y0_bf16 (and x0_bf16).
Atomic sums depend on arrival order and are not hashed: logdet, d_an_logs / d_an_bias / d_w_ic on the atomics route, what
gt_boundary_param_reduce adds to them on the partials route, and the five-launch kernels' logdet / dlogs / dbias / dW; compare them
(--save / --against) with a second run of the same tree as the yardstick.
No launch is repeated or retried: run it under the caller's timeout."""
import ctypes
import hashlib
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import torch

H, C, HALF, NL, NB = 192, 160, 80, 4, 3
CAN = 768.0
# name: (squeezed lengths, squeezed T, ragged rows + folded squeeze / unsqueeze)      (tests/test_wn_boundary_fp64_gpu.py LAYOUTS)
LAYOUTS = {"ragged": ([37, 1, 2, 60, 13], 60, True), "uniform": ([37, 1, 2, 60, 13], 140, False),
           "many": ([1 + (i % 2) for i in range(300)], 2, True)}
PASSES = [(layout, ss) for layout in LAYOUTS for ss in (False, True)]
ROW_IN = {"fwd": ("acts", "y", "x_in"), "bwd": ("dh", "dx_in", "x", "dz_in", "logs_raw", "y"), "rev": ("acts", "z", "x_in")}
ROW_OUT = {"fwd": ("wn_out", "logs_raw", "z", "y_next", "y0_bf16", "h_next"), "bwd": ("dx_out", "dout", "dwn_out", "via_skip"), "rev": ("x", "h_next")}
BCT_OUT = {"fwd": "z_bct", "bwd": "dx_bct", "rev": "x_bct"}
ACC = (("d_an_logs", C), ("d_an_bias", C), ("d_w_ic", 16))


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def redrawn(t, rc, tag):
    """a tensor of t's shape and type drawn from a seed of the tag's, zero on masked rows"""
    g = torch.Generator().manual_seed(zlib.crc32(tag.encode()))
    return (torch.randn(t.shape, generator=g) * 0.5 * rc.rowmask.cpu()[:, None]).to(t.dtype).to(t.device)


def prior_of(n, dev, scale=1.0):
    return ((0.5 + 0.25 * (torch.arange(n) % 7)) * scale).float().to(dev)


def record(layout, ss, dev):
    """one 3-block pass -> (rows context, decoder, dlogdet, {kind: [kw of every launch]})"""
    from fill import fill_module
    from glow_tts_amd import flow_impl, models, modules, ops, wgrad
    from glow_tts_amd._lib import call
    lens, T, ragged = LAYOUTS[layout]
    B = len(lens)
    dec = fill_module(models.FlowSpecDecoder(80, H, 5, 1, NB, NL, p_dropout=0.05, sigmoid_scale=ss), "decoder.").to(dev).train()
    modules.prepare_all(dec)
    rc = ops.RowsCtx(torch.tensor(lens, dtype=torch.int32, device=dev), T, lengths_host=lens if ragged else None, round_to=8)
    g = torch.Generator().manual_seed(17 + B)
    fm = (torch.arange(2 * T)[None, :] < 2 * torch.tensor(lens)[:, None]).unsqueeze(1).float().to(dev)
    rn = lambda *s: torch.randn(*s, generator=g).to(dev)
    y, dz, zl = rn(B, HALF, 2 * T) * fm, rn(B, HALF, 2 * T) * fm, rn(B, HALF, 2 * T) * fm
    dlogdet = rn(B) * 0.1
    st = flow_impl._st(dev)

    def sq(t):
        r = torch.empty(rc.R, C, device=dev)
        call.gt_squeeze_rows_f32(t, r, rc.lengths, B, HALF, 2 * T, rc.Tp, rc.row0, st)
        return r

    logdet = torch.zeros(B, device=dev)
    flow_impl.BOUNDARY_TRACE = trace = []
    try:
        if ragged:
            _, blocks = flow_impl.decoder_fwd_fused(rc, dec, None, [None] * NB, logdet, True, 5, y_bct=y, z_bct=torch.zeros_like(y))
            with wgrad.WgradQueue(dev, site=dec):
                flow_impl.decoder_bwd_fused(rc, dec, blocks, None, dlogdet, False, dz_bct=dz, dx_bct=torch.zeros_like(y))
            dec.eval()
            flow_impl.decoder_rev_fused(rc, dec, None, [None] * NB, z_bct=zl, x_bct=torch.zeros_like(y))
        else:
            _, blocks = flow_impl.decoder_fwd_fused(rc, dec, sq(y), [None] * NB, logdet, True, 5)
            with wgrad.WgradQueue(dev, site=dec):
                flow_impl.decoder_bwd_fused(rc, dec, blocks, sq(dz), dlogdet, False)
            dec.eval()
            flow_impl.decoder_rev_fused(rc, dec, sq(zl), [None] * NB)
    finally:
        flow_impl.BOUNDARY_TRACE = None
    torch.cuda.synchronize()
    launches = {kind: [kw for n, _, kw in trace if n == "gt_wn_boundary_" + kind] for kind in ("fwd", "bwd", "rev")}
    assert all(len(v) == NB + 1 for v in launches.values())
    return rc, dec, dlogdet, launches, blocks


def reissue(kind, kw, rc, dev, tag, route=None):
    """one recorded launch again on redrawn operands and pre-filled buffers -> ({hashed output: tensor}, {atomic sum: tensor})"""
    from glow_tts_amd import _lib
    from glow_tts_amd._lib import call
    L = _lib.lib()
    kw = dict(kw)
    out, sums = {}, {}
    for k in ROW_IN[kind]:
        if kw.get(k) is not None:
            kw[k] = redrawn(kw[k], rc, f"{tag} {k}")
    if kw.get("acts") is not None:
        kw["ldacts"] = kw["acts"].stride(0)
    for k in ROW_OUT[kind]:
        if kw.get(k) is not None:
            kw[k] = out[k] = torch.full_like(kw[k], CAN)
    if kw.get("via_skip") is not None:
        kw["ldvs"] = kw["via_skip"].stride(0)
    k = BCT_OUT[kind]
    if kw.get(k) is not None:
        kw[k] = out[k] = torch.zeros_like(kw[k])                          # pre-zeroed by the caller
    if kind == "fwd":
        kw["logdet"] = sums["logdet"] = prior_of(rc.B, dev)
    tab = None
    if kind == "bwd" and kw.get("dh") is not None:
        for k, n in ACC:
            kw[k] = sums[k] = prior_of(n, dev, 3.0)
        if route == "partials":
            n_wg, PG = (rc.R + 63) // 64, L.gt_boundary_param_partials()
            kw["pg_partial"] = out["pg_partial"] = torch.full((n_wg * PG,), float("nan"), device=dev)
            tab = torch.tensor([sums[k].data_ptr() for k, _ in ACC], dtype=torch.int64).to(dev)
        else:
            kw["pg_partial"] = None
    cls = {"fwd": _lib.BoundaryFwdArgs, "bwd": _lib.BoundaryBwdArgs, "rev": _lib.BoundaryRevArgs}[kind]
    args = _lib.fill_args(cls, **{k: v for k, v in kw.items() if v is not None})
    _lib.check(getattr(L, "gt_wn_boundary_" + kind)(ctypes.byref(args), _lib.current_stream(dev)), kind)
    if tab is not None:
        call.gt_boundary_param_reduce(out["pg_partial"], (rc.R + 63) // 64, 1, tab, _lib.current_stream(dev))
    torch.cuda.synchronize()
    return out, sums


def five_launch(kw, rc, dlogdet, ss, dev):
    """gt_coupling_fwd / _bwd / _rev and gt_actnorm_invconv_fwd / _bwd / _rev on the operands of one recorded forward launch"""
    from glow_tts_amd import flow_impl
    from glow_tts_amd._lib import call
    st, B, R = flow_impl._st(dev), rc.B, rc.R
    g = torch.Generator().manual_seed(3)
    f32 = dict(dtype=torch.float32, device=dev)
    m = (torch.randn(R, HALF, generator=g) * 0.5).to(dev)
    outp = torch.cat([m, kw["logs_raw"]], 1).contiguous()
    out, sums = {}, {}
    z, logdet = torch.full((R, C), CAN, **f32), prior_of(B, dev)
    call.gt_coupling_fwd(outp, kw["y"], z, rc.rowmask, logdet, B, R, C, rc.Tp, rc.row0, int(ss), st)
    dz = torch.randn(R, C, generator=g).to(dev).contiguous()
    dx, dout = torch.full((R, C), CAN, **f32), torch.full((R, C), CAN, dtype=torch.bfloat16, device=dev)
    call.gt_coupling_bwd(outp, kw["y"], dz, dlogdet, rc.rowmask, dx, dout, B, R, C, rc.Tp, rc.row0, int(ss), st)
    xr = torch.full((R, C), CAN, **f32)
    call.gt_coupling_rev(outp, z, xr, rc.rowmask, R, C, int(ss), st)
    out.update({"gt_coupling_fwd z": z, "gt_coupling_bwd dx": dx, "gt_coupling_bwd dout_bf16": dout, "gt_coupling_rev x": xr})
    sums["gt_coupling_fwd logdet"] = logdet
    lgd, bsd, Wdv = kw["an_logs"].detach().reshape(-1).contiguous(), kw["an_bias"].detach().reshape(-1).contiguous(), kw["w_ic"].detach().contiguous()
    scal = kw["scal"].contiguous()
    yk, y0 = torch.full((R, C), CAN, **f32), torch.full((R, HALF), CAN, dtype=torch.bfloat16, device=dev)
    ld2 = prior_of(B, dev)
    call.gt_actnorm_invconv_fwd(kw["z"], yk, y0, HALF, lgd, bsd, Wdv, scal, rc.rowmask, rc.lengths, ld2, B, R, C, st)
    xk, x0 = torch.full((R, C), CAN, **f32), torch.full((R, HALF), CAN, dtype=torch.bfloat16, device=dev)
    call.gt_actnorm_invconv_rev(yk, xk, x0, HALF, lgd, bsd, scal, rc.rowmask, R, C, st)
    dy = torch.randn(R, C, generator=g).to(dev).contiguous()
    dxk = torch.full((R, C), CAN, **f32)
    acc = {k: prior_of(n, dev, 3.0) for k, n in ACC}
    call.gt_actnorm_invconv_bwd(kw["z"], dy, dxk, lgd, bsd, Wdv, scal, rc.rowmask, rc.lengths, dlogdet, acc["d_an_logs"], acc["d_an_bias"], acc["d_w_ic"],
                                B, R, C, st)
    torch.cuda.synchronize()
    out.update({"gt_actnorm_invconv_fwd y": yk, "gt_actnorm_invconv_fwd y0_bf16": y0, "gt_actnorm_invconv_rev x": xk,
                "gt_actnorm_invconv_rev x0_bf16": x0, "gt_actnorm_invconv_bwd dx": dxk})
    sums["gt_actnorm_invconv_fwd logdet"] = ld2
    sums.update({"gt_actnorm_invconv_bwd " + n: acc[k] for k, n in (("d_an_logs", "dlogs"), ("d_an_bias", "dbias"), ("d_w_ic", "dW"))})
    return out, sums


def run_pass(layout, ss):
    """-> (pass name, [lines of the listing], {name: atomic sum on the host})"""
    dev = torch.device("cuda:0")
    name = f"{layout} ss={int(ss)}"
    rc, dec, dlogdet, launches, blocks = record(layout, ss, dev)
    lines, sums = [], {}
    for kind in ("fwd", "bwd", "rev"):
        for i, kw in enumerate(launches[kind]):
            routes = ("partials", "atomics") if kind == "bwd" and kw.get("dh") is not None else (None,)
            for route in routes:
                tag = f"{kind}[{i}]" + (f" {route}" if route else "")
                out, s = reissue(kind, kw, rc, dev, f"{name} {kind}[{i}]", route)
                lines += [f"{name} | {tag} {k} {sha(t)}" for k, t in out.items()]
                sums.update({f"{tag} {k}": t.cpu() for k, t in s.items()})
    out, s = five_launch({k: (redrawn(v, rc, f"{name} five {k}") if k in ("logs_raw", "y", "z") else v) for k, v in launches["fwd"][1].items()},
                         rc, dlogdet, ss, dev)
    lines += [f"{name} | {k} {sha(t)}" for k, t in out.items()]
    sums.update({k: t.cpu() for k, t in s.items()})
    return name, lines, sums


def listing():
    """[(lines of the listing, pass name, atomic sums)]: the text tests/test_wn_boundary_trace_gpu.py compares"""
    return [(lines, name, sums) for name, lines, sums in (run_pass(layout, ss) for layout, ss in PASSES)]


def main(argv):
    save = argv[argv.index("--save") + 1] if "--save" in argv else None
    against = argv[argv.index("--against") + 1] if "--against" in argv else None
    yard = argv[argv.index("--yardstick") + 1] if "--yardstick" in argv else None
    if save:
        os.makedirs(save, exist_ok=True)
    for lines, name, sums in listing():
        print("\n".join(lines), flush=True)
        fname = name.replace(" ", "_").replace("=", "") + ".pt"
        if save:
            torch.save(sums, os.path.join(save, fname))
        if against:
            ref = torch.load(os.path.join(against, fname))
            ref2 = torch.load(os.path.join(yard, fname)) if yard else None
            for n, t in sums.items():
                d = float((t - ref[n]).abs().max())
                line = f"# sum {name} | {n} max|sum - saved| {d:.3e}  max|saved| {float(ref[n].abs().max()):.3e}"
                if ref2 is not None:
                    y = float((ref2[n] - ref[n]).abs().max())
                    line += f"  yardstick max|saved2 - saved| {y:.3e}" + ("  OVER" if d > 2 * y else "")
                print(line, flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
