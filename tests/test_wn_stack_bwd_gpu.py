"""gt_wn_stack_bwd in the 64-row form (the one the benchmark's decoder runs) against the per-layer kernels, bit for bit.

The equality tests in test_decoder_gpu.py use a few hundred rows, which the launcher gives to the 32-row form.  Here a
cfg-2-shaped batch (32 utterances, at most 800 mel frames, about 9 k squeezed rows, well over 80 tiles) takes the 64-row
form: d h0, d cond and every parameter gradient must be EQUAL, for each conditioning mode, dropout on, 1..4 layers."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
from fill import fill_module  # noqa: E402

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def cfg2_rows():
    from glow_tts_amd import ops
    g = torch.Generator().manual_seed(1234)
    t_y = torch.randint(150, 401, (32,), generator=g) * 2
    t_y[0] = 800
    lens = [int(v) // 2 for v in t_y]
    return ops.RowsCtx(torch.tensor(lens, dtype=torch.int32, device=dev()), 400, lengths_host=lens, round_to=512)


@pytest.mark.parametrize("n", [1, 2, 3, 4])
@pytest.mark.parametrize("mode", ["none", "speaker", "per_row"])
def test_wn_stack_backward_64_row_form_is_bit_identical(built, mode, n):
    from glow_tts_amd import _lib, flow_impl, modules, wgrad
    H = 192
    gin = 256 if mode == "speaker" else 0
    wn = fill_module(modules.WN(160, H, 5, 1, n, gin, 0.05), "wn.").to(dev())
    modules.prepare_all(wn)
    rc = cfg2_rows()
    assert rc.R > 8000
    assert _lib.lib().gt_wn_stack_row_blocks(rc.R, n, 0) == 2            # the 64-row form
    g = torch.Generator().manual_seed(40 + n)
    h0 = ((torch.randn(rc.R, H, generator=g)).to(dev()) * rc.rowmask[:, None]).to(torch.bfloat16)
    dskip = ((torch.randn(rc.R, H, generator=g)).to(dev()) * rc.rowmask[:, None]).to(torch.bfloat16)
    cond = None
    if mode == "speaker":
        cond = (torch.randn(rc.B, 2 * H * n, generator=g) * 0.3).to(dev())
    elif mode == "per_row":
        cond = (torch.randn(rc.R, 2 * H * n, generator=g) * 0.3).to(dev())
    res = []
    for stack in (True, False):
        wn.set_stack(stack, stack)
        try:
            out, saved = flow_impl.wn_fwd(rc, wn, h0, cond, True, 77, cond_per_row=mode == "per_row")
            with wgrad.WgradQueue(dev(), site=wn):
                dh0, grads, dcond = flow_impl.wn_bwd(rc, wn, saved, dskip, want_dcond=cond is not None, cond_per_row=mode == "per_row")
        finally:
            wn.set_stack(True, True)
        torch.cuda.synchronize()
        res.append((dh0.clone(), None if dcond is None else dcond.clone(), {id(k): v.clone() for k, v in grads.items()}))
    (d1, c1, g1), (d2, c2, g2) = res
    assert torch.equal(d1, d2)
    assert (c1 is None) == (cond is None)
    if c1 is not None:
        assert torch.equal(c1, c2)
    assert g1.keys() == g2.keys() and len(g1) > 0
    for k in g1:
        assert torch.equal(g1[k], g2[k])
