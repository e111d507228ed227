"""The two forms of the weight-norm backward (csrc/conv_wgrad.hip): the 16-byte form (Cin % 4 == 0; part, v, dv 16-byte aligned) against
the 4-byte form on the same values — the 4-byte form is forced by handing it copies of part, v and dv at a +4-byte offset — bit for bit
in dv, dg and dbias; the batched launch's job lookup against a host-side search; and the 16-byte form against float64 of its own fp32
inputs under the rule of oracle/rows64.py (gamma_K * S carried through the weight-norm map, relative L2 <= 2e-5, a planted defect that
must miss by >= 3x), as tests/test_wgrad_fp64_gpu.py applies it.

Shapes (Cout, Cin, taps), the smallest at which the forms can part: n/4 = 240 chunks, the last pass partly masked; fewer than 64
chunks; Cout no multiple of the rows per workgroup; n = 2304, the LDS limit (three passes, three rows per workgroup); Cin % 4 != 0,
which takes the 4-byte form on its own."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from oracle import rows64

pytestmark = pytest.mark.gpu

SHAPES = [(384, 192, 5), (192, 80, 1), (6, 192, 1), (192, 768, 3), (16, 10, 3)]
SLABS = [1, 2, 3, 5]


def dev():
    return torch.device("cuda:0")


def _at(t, off):
    """a copy of `t` whose first element sits `off` floats past a 16-byte boundary (torch allocations are 512-byte aligned)"""
    buf = torch.empty(t.numel() + 4, dtype=torch.float32, device=t.device)
    assert buf.data_ptr() % 16 == 0
    out = buf[off:off + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4 * off
    return out


def _values(Cout, Cin, taps, S, seed):
    g = torch.Generator().manual_seed(seed)
    n = Cin * taps
    d = {
        "ws": torch.randn(S * taps * Cout * Cin + S * Cout, generator=g),       # slab partials [S][taps][Cout][Cin] | bias partials [S][Cout]
        "v": torch.randn(Cout, Cin, taps, generator=g),
        "g": torch.randn(Cout, generator=g),
        "dv0": torch.randn(Cout, Cin, taps, generator=g),                      # what the destinations hold (accumulate = 1)
        "dg0": torch.randn(Cout, generator=g),
        "db0": torch.randn(Cout, generator=g),
    }
    d["inv"] = (1.0 / d["v"].reshape(Cout, n).double().norm(dim=1)).float()
    return {k: t.to(dev()) for k, t in d.items()}


def _single(L, d, Cout, Cin, taps, S, off, accumulate, use_g, use_bias):
    """gt_weightnorm_bwd on the values `d`, part / v / dv at `off` floats past a 16-byte boundary -> (dv, dg, dbias) on the CPU"""
    from glow_tts_amd import _lib
    R = 64 * S
    s_lib = ctypes.c_int(0)
    L.gt_conv_wgrad_workspace_bytes(R, Cin, Cout, taps, ctypes.byref(s_lib))
    assert s_lib.value == S, (s_lib.value, S)
    ws, v, dv = _at(d["ws"], off), _at(d["v"], off), _at(d["dv0"], off)
    dg, db = d["dg0"].clone(), d["db0"].clone()
    _lib.check(L.gt_weightnorm_bwd(_lib.ptr(ws), R, _lib.ptr(v), _lib.ptr(d["g"]) if use_g else None,
                                   _lib.ptr(d["inv"]) if use_g else None, _lib.ptr(dv), _lib.ptr(dg) if use_g else None,
                                   _lib.ptr(db) if use_bias else None, Cout, Cin, taps, accumulate, _lib.current_stream(dev())),
               "gt_weightnorm_bwd")
    torch.cuda.synchronize()
    return dv.cpu(), dg.cpu(), db.cpu()


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("Cout,Cin,taps", SHAPES)
def test_wide_form_equals_narrow_form_bit_for_bit(built, Cout, Cin, taps):
    from glow_tts_amd import _lib
    L = _lib.lib()
    for S in SLABS:
        d = _values(Cout, Cin, taps, S, seed=Cout + 7 * Cin + taps + 1000 * S)
        for accumulate, use_g, use_bias in itertools.product((0, 1), (True, False), (True, False)):
            wide = _single(L, d, Cout, Cin, taps, S, 0, accumulate, use_g, use_bias)       # (16, 10, 3): the 4-byte form here too
            narrow = _single(L, d, Cout, Cin, taps, S, 1, accumulate, use_g, use_bias)
            tag = f"{Cout}x{Cin}x{taps} S={S} accumulate={accumulate} g={use_g} bias={use_bias}"
            for name, a, b in zip(("dv", "dg", "dbias"), wide, narrow):
                assert _same_bits(a, b), f"{tag}: {name} differs in {(a != b).sum().item()} of {a.numel()} elements"
            # the launch wrote what it should have: dv always, dg / dbias only when asked for
            assert not torch.equal(wide[0], d["dv0"].cpu())
            assert torch.equal(wide[1], d["dg0"].cpu()) != use_g and torch.equal(wide[2], d["db0"].cpu()) != use_bias


def _batched_jobs(seed):
    """>= 70 small jobs of mixed shapes and slab counts; Cout values that leave row_start off every multiple of 4"""
    rng = np.random.RandomState(seed)
    shapes = [(6, 192, 1), (5, 16, 3), (3, 10, 3), (7, 80, 1), (9, 48, 5), (2, 192, 5), (11, 8, 1), (1, 20, 3)]
    jobs = []
    for i in range(75):
        Cout, Cin, taps = shapes[rng.randint(len(shapes))]
        jobs.append((Cout, Cin, taps, int(rng.randint(1, 6)), bool(i % 3), bool(i % 2), int(i % 5 == 0)))
    return jobs


def test_batched_lookup_matches_host_search(built):
    """One batched launch over 75 jobs (more than one round of 64 lanes) against one single launch per job: the rows of every job
    must have gone through that job's descriptor.  Even jobs are 16-byte aligned, odd ones sit at +4 bytes."""
    from glow_tts_amd import _lib, wgrad
    L = _lib.lib()
    jobs = _batched_jobs(5)
    table = np.zeros(len(jobs), dtype=wgrad.WNB)
    keep, expect, row, max_n = [], [], 0, 1
    starts = []
    for i, (Cout, Cin, taps, S, use_g, use_bias, accumulate) in enumerate(jobs):
        d = _values(Cout, Cin, taps, S, seed=100 + i)
        off = i & 1
        ws, v, dv = _at(d["ws"], off), _at(d["v"], off), _at(d["dv0"], off)
        dg, db = d["dg0"].clone(), d["db0"].clone()
        keep.append((d, ws, v, dv, dg, db))
        t = table[i]
        t["part"], t["part_bias"] = ws.data_ptr(), ws.data_ptr() + 4 * S * taps * Cout * Cin
        t["v"], t["dv"] = v.data_ptr(), dv.data_ptr()
        if use_g:
            t["g"], t["inv_norm"], t["dg"] = d["g"].data_ptr(), d["inv"].data_ptr(), dg.data_ptr()
        if use_bias:
            t["dbias"] = db.data_ptr()
        t["S"], t["Cout"], t["Cin"], t["taps"], t["row_start"], t["accumulate"] = S, Cout, Cin, taps, row, accumulate
        starts.append(row)
        row += Cout
        max_n = max(max_n, Cin * taps)
        # the same job alone, through the single form (its S comes from R)
        expect.append(_single(L, d, Cout, Cin, taps, S, off, accumulate, use_g, use_bias) if S <= 16 else None)
    assert any(s % 4 for s in starts) and len(jobs) >= 70
    # host-side search: the job of every row of the launch
    owner = np.searchsorted(np.array(starts), np.arange(row), side="right") - 1
    assert all(starts[j] <= r < starts[j] + jobs[j][0] for r, j in enumerate(owner))
    dtab = torch.from_numpy(table.view(np.uint8).reshape(-1).copy()).to(dev())
    _lib.check(L.gt_weightnorm_bwd_batched(_lib.ptr(dtab), len(jobs), row, max_n, _lib.current_stream(dev())), "gt_weightnorm_bwd_batched")
    torch.cuda.synchronize()
    for i, ((d, ws, v, dv, dg, db), exp) in enumerate(zip(keep, expect)):
        for name, a, b in zip(("dv", "dg", "dbias"), (dv.cpu(), dg.cpu(), db.cpu()), exp):
            assert _same_bits(a, b), f"job {i} {jobs[i]}: {name} differs from the single launch of the same job"


@pytest.mark.parametrize("Cout,Cin,taps", SHAPES[:4])
def test_wide_form_vs_float64(built, Cout, Cin, taps):
    from glow_tts_amd import _lib
    L = _lib.lib()
    u = rows64.RHO["f32"]
    for S, accumulate in ((1, 0), (2, 1), (5, 1)):
        d = _values(Cout, Cin, taps, S, seed=Cout + Cin + taps + S)
        nW = S * taps * Cout * Cin
        part = rows64.t64(d["ws"][:nW]).reshape(S, taps, Cout, Cin)
        pb = rows64.t64(d["ws"][nW:]).reshape(S, Cout)
        dW, SW = part.sum(0), part.abs().sum(0)                                  # K = S terms per element
        bad_dW = rows64.drop_weight_entry(dW)                                    # planted defect: one (tap, ci) column of dW gone
        prior = {k: rows64.t64(d[k]) for k in ("dv0", "dg0", "db0")}

        def with_prior(ref, bnd, p):
            return (ref + p, bnd + u * (ref.abs() + p.abs())) if accumulate else (ref, bnd)

        for use_g in (True, False):
            dv, dg, db = _single(L, d, Cout, Cin, taps, S, 0, accumulate, use_g, True)
            tag = f"weight-norm backward {Cout}x{Cin}x{taps} S={S} accumulate={accumulate} {'wn' if use_g else 'plain'}"
            if use_g:
                rdv, rdg, bdv, bdg = rows64.weightnorm_bwd(dW, SW, S, d["v"], d["g"], d["inv"])
                xdv, xdg, _, _ = rows64.weightnorm_bwd(bad_dW, SW, S, d["v"], d["g"], d["inv"])
                rdg, bdg = with_prior(rdg, bdg, prior["dg0"])
                xdg = xdg + prior["dg0"] if accumulate else xdg
                rows64.check_with_control(tag + " dg", dg, rdg, bdg, xdg)
            else:
                rdv, bdv, xdv = dW.permute(1, 2, 0), rows64.gamma(S) * SW.permute(1, 2, 0), bad_dW.permute(1, 2, 0)
            rdv, bdv = with_prior(rdv, bdv, prior["dv0"])
            xdv = xdv + prior["dv0"] if accumulate else xdv
            rows64.check_with_control(tag + " dv", dv, rdv, bdv, xdv)
            rdb, bdb = with_prior(pb.sum(0), rows64.gamma(S) * pb.abs().sum(0), prior["db0"])
            xdb = pb[1:].sum(0) + (prior["db0"] if accumulate else 0) if S > 1 else torch.zeros_like(rdb)
            rows64.check_with_control(tag + " dbias", db, rdb, bdb, xdb)
