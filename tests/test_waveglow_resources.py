"""The WaveGlow kernels (csrc/waveglow.hip) as the compiler built them: two kernels, neither with scratch or spilled
registers.  What DESIGN.md 4.28 states:

  gt_wg_gate      dynamic LDS of gt_wg_gate_lds_bytes(C, 3, dil) = (128 + 2 dil) 144 bytes, 55 296 at dilation 128: two workgroups a CU
                  within its 160 KB, and the registers to match — at most 256 (128 of them the two accumulator tiles of four 32-row
                  blocks), two waves per SIMD
  gt_wg_boundary  no LDS, at most 128 registers: four waves per SIMD or more

An edit that grows any of these fails here.  Parsing and the per-kernel checks: tests/kernel_resources.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_resources as KR  # noqa: E402


def test_waveglow_kernel_resources(built):
    from glow_tts_amd import _lib
    L = _lib.lib()
    kernels = {"gt_wg_gate_kernel": (0, 2), "gt_wg_boundary_kernel": (0, 4)}            # the gate's LDS is dynamic: checked below
    seen = KR.check_kernels("waveglow", kernels, max_regs=256, resident=2, at_least=True)
    for name, (f, line) in seen.items():
        assert f["Dynamic Stack"] == "False", line
    f, line = seen["gt_wg_gate_kernel"]
    assert f["Occupancy [waves/SIMD]"] == "2" and 128 < int(f["VGPRs"]) + int(f["AGPRs"]) <= 256, line
    f, line = seen["gt_wg_boundary_kernel"]
    assert int(f["VGPRs"]) + int(f["AGPRs"]) <= 128, line
    worst = L.gt_wg_gate_lds_bytes(512, 3, 128)
    assert worst == 55296 and 2 * worst <= KR.CU_LDS_BYTES < 3 * worst               # two workgroups a CU at the deepest layer
    assert 2 * L.gt_wg_gate_lds_bytes(64, 3, 1) <= KR.CU_LDS_BYTES
