"""The packed bf16 weight images of a cfg-2 decoder, decoded back to dense [taps][Cout][Cin] (oracle/rows64.py), must EQUAL what the
packer is specified to write, bf16(fp32(v * fp32(g * inv_norm))) with the kernel's own inv_norm, padding entries included (zero) —
for every conv, through the one-launch packing of prepare_all (gt_pack_conv_weights_multi) and through gt_pack_conv_weights.  The fp64
tests of the decoder kernels take their weights from decoded images; this is what ties those images to the module's parameters."""
import os
import sys
import types

import numpy as np
import pytest
import torch

from oracle import rows64

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
from fill import fill_module  # noqa: E402

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def _inv_of(entry, owners):
    """inv_norm rows of an entry's v: its own (PackedConv) or, for a window of a concatenated GEMM (PackSlice, which writes none),
    the rows of the norm entry of the same parameter (same kernel, same row: the same fp32 value)"""
    v, g, pc = entry
    if g is None:
        return None
    if pc.inv_norm is not None:
        return pc.inv_norm
    n = v[0].numel() * v.element_size()
    for lo, hi, inv in owners:
        if lo <= v.data_ptr() < hi:
            r0 = (v.data_ptr() - lo) // n
            return inv[r0:r0 + v.shape[0]]
    raise AssertionError("no inv_norm for a weight-normed slice")


def _check_images(tag, entry, inv, full):
    v, g, pc = entry
    Cout, Cin, taps = v.shape
    want = rows64.packed_weights(v, g, None if g is None else inv)
    flags = pc.flags
    fwd = rows64.decode_fwd(pc.fwd, Cout, Cin, taps, pc.Np_f, pc.Kp_f, flags)
    dgr = rows64.decode_dgrad(pc.dgrad, Cout, Cin, taps, pc.Np_d, pc.Kp_d, flags)
    assert torch.equal(fwd, want), (tag, int((fwd != want).sum()))
    assert torch.equal(dgr, want), (tag, int((dgr != want).sum()))
    if full:                                                   # a whole image: everything but the weights is padding, and zero
        for img, Np, Kp, fr in ((pc.fwd, pc.Np_f, pc.Kp_f, flags & 2), (pc.dgrad, pc.Np_d, pc.Kp_d, flags & 4)):
            assert img.numel() == taps * Np * Kp
            nz = int((rows64.decode_image(img, taps, Np, Kp, bool(fr)) != 0).sum())
            assert nz == int((want != 0).sum()), (tag, nz)


def test_decoder_images_equal_the_packers_contract(built):
    from glow_tts_amd import models, modules, ops
    dec = fill_module(models.FlowSpecDecoder(80, 192, 5, 1, 12, 4, p_dropout=0.05), "decoder.").to(dev())
    modules.prepare_all(dec)
    entries = dec._pack_plan.keep
    torch.cuda.synchronize()
    owners = [(v.data_ptr(), v.data_ptr() + v.numel() * v.element_size(), pc.inv_norm) for v, g, pc in entries
              if g is not None and pc.inv_norm is not None]
    seen = set()
    n_img = 0
    for i, e in enumerate(entries):
        v, g, pc = e
        inv = _inv_of(e, owners)
        if g is not None and pc.inv_norm is not None:          # the norms themselves: float64 1/||v|| within the accumulation bound
            vv = rows64.t64(v).reshape(v.shape[0], -1)
            ss = (vv * vv).sum(1)
            want = ss.rsqrt()
            bound = 0.5 * rows64.gamma(vv.shape[1]) * want + 2 * rows64.RHO["f32"] * want
            r = rows64.check(f"inv_norm {tuple(v.shape)}", pc.inv_norm, want, bound)
            assert r.ok, str(r)
        if pc.fwd is None:                                     # norm only: the weights are packed by a window entry
            continue
        full = isinstance(pc, ops.PackedConv)
        seen.add(pc.flags)
        _check_images(f"multi #{i} {tuple(v.shape)} flags {pc.flags}", e, inv, full)
        # the same conv through the single-conv packer, into fresh zeroed images
        fresh = types.SimpleNamespace(Cout=pc.Cout, Cin=pc.Cin, taps=pc.taps, Np_f=pc.Np_f, Kp_f=pc.Kp_f, Np_d=pc.Np_d, Kp_d=pc.Kp_d,
                                      flags=pc.flags, km=1, fwd=torch.zeros_like(pc.fwd), dgrad=torch.zeros_like(pc.dgrad),
                                      inv_norm=None if g is None else torch.zeros(v.shape[0], device=dev()))
        modules._pack_one(fresh, v, g)      # (a window gets an inv_norm buffer here: this kernel's own reduction order may differ)
        torch.cuda.synchronize()
        inv1 = fresh.inv_norm
        _check_images(f"single #{i} {tuple(v.shape)} flags {pc.flags}", (v, g, fresh), inv1, full)
        n_img += 1
    assert {0, 6, 22} <= seen, seen                            # plain, fragment order, fragment order + [16 | 16] gate interleave
    print(f"{n_img} convs: decoded images equal the packer's contract (flags {sorted(seen)})")


# ----------------------------------------------------------------------------- the text encoder's shapes, every packing kernel
# (Cout, Cin, taps, weight-normed, PackedConv keywords): the FFN's two convs (768 x 192 x 3; 192 x 768 x 3 = 2304 elements per row,
# exactly the documented limit of the 8-row kernel), the prenet, qkv, the duration predictor and its 8-wide proj_pad, a gate conv
# with the [32 | 32] interleave gate == 1 reads (flag 1), and a bf16x3 conv (flag 8: one row per workgroup only)
ENC_CONVS = [(768, 192, 3, False, {}), (192, 768, 3, False, {}), (192, 192, 5, True, {}), (576, 192, 1, False, {}), (256, 192, 3, False, {}),
             (8, 256, 1, False, {}), (192, 80, 1, True, {}), (384, 192, 5, True, dict(gate=True)), (192, 192, 1, False, dict(split3=True))]


def _split_check(tag, v, pc):
    """flag 8: both images are plain images of [w_hi | w_lo | w_hi] along the reduction axis, zero elsewhere"""
    Cout, Cin, _ = v.shape
    vf = v.detach().cpu().float().numpy()[:, :, 0]
    hi = rows64.bf16_round(vf)
    lo = rows64.bf16_round((vf - hi.astype(np.float32)).astype(np.float32))
    want_f = torch.from_numpy(np.concatenate([hi, lo, hi], 1))[None]              # [1][Cout][3 Cin]
    want_d = torch.from_numpy(np.concatenate([hi.T, lo.T, hi.T], 1))[None]        # [1][Cin][3 Cout]
    fwd = rows64.decode_fwd(pc.fwd, Cout, 3 * Cin, 1, pc.Np_f, pc.Kp_f, 0)
    dgr = rows64.decode_fwd(pc.dgrad, Cin, 3 * Cout, 1, pc.Np_d, pc.Kp_d, 0)
    assert torch.equal(fwd, want_f), (tag, int((fwd != want_f).sum()))
    assert torch.equal(dgr, want_d), (tag, int((dgr != want_d).sum()))
    for img, Np, Kp, want in ((pc.fwd, pc.Np_f, pc.Kp_f, want_f), (pc.dgrad, pc.Np_d, pc.Kp_d, want_d)):
        assert int((rows64.decode_image(img, 1, Np, Kp, False) != 0).sum()) == int((want != 0).sum()), tag


@pytest.mark.parametrize("group8", [0, 1, 2])
def test_encoder_shapes_through_every_multi_conv_packer(built, group8):
    """gt_pack_conv_weights_multi with group8 = 0 (one row per workgroup: every conv, the split one included), 1 (8 rows, rows of up to
    2304 elements) and 2 (8 rows, up to 1024): each image equals rows64.packed_weights with the kernel's own inv_norm, padding zero."""
    from glow_tts_amd import _lib, ops
    g = torch.Generator().manual_seed(group8)
    convs = [c for c in ENC_CONVS if group8 == 0 or (not c[4].get("split3") and c[1] * c[2] <= (2304 if group8 == 1 else 1024))]
    assert group8 == 2 or any(c[1] * c[2] == 2304 for c in convs)
    entries = []
    for Cout, Cin, taps, wn, kw in convs:
        v = (torch.randn(Cout, Cin, taps, generator=g) / (Cin * taps) ** 0.5).to(dev())
        gg = (torch.rand(Cout, generator=g) + 0.5).to(dev()) if wn else None
        entries.append((v, gg, ops.PackedConv(Cout, Cin, taps, device=dev(), **kw)))
    arr = (_lib.PackDesc * len(entries))()
    row = 0
    for d, (v, gg, pc) in zip(arr, entries):
        d.v, d.g = v.data_ptr(), (gg.data_ptr() if gg is not None else None)
        d.pack_fwd, d.pack_dgrad, d.inv_norm = pc.fwd.data_ptr(), pc.dgrad.data_ptr(), pc.inv_norm.data_ptr()
        d.Cout, d.Cin, d.taps = pc.Cout, pc.Cin, pc.taps
        d.Np_fwd, d.Kp_fwd, d.Np_dgrad, d.Kp_dgrad, d.gate, d.row_start = pc.Np_f, pc.Kp_f, pc.Np_d, pc.Kp_d, pc.flags, row
        row += pc.Cout
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev())
    _lib.call.gt_pack_conv_weights_multi(table, len(entries), row, group8, _lib.current_stream(dev()))
    torch.cuda.synchronize()
    seen = set()
    for v, gg, pc in entries:
        tag = f"group8={group8} {tuple(v.shape)} flags {pc.flags}"
        seen.add(pc.flags)
        if pc.flags & 8:
            _split_check(tag, v, pc)
        else:
            _check_images(tag, (v, gg, pc), pc.inv_norm, True)
    assert seen == ({0, 1, 8} if group8 == 0 else {0, 1}), seen
