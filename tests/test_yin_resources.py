"""The pitch front end's kernel (csrc/yin_front.hip) as the compiler built it: no scratch, no spilled registers, and the LDS footprint
and occupancy DESIGN.md 4.18 states — the samples a 16-frame tile reads ((16 + 3) * 256 + 512 floats) plus a ring of four frames'
difference functions (4 * 512 floats) = 29 696 bytes per workgroup of two waves, so that five workgroups (at least two) are resident
on a CU's 160 KB, within a register budget (at most 256) that allows them.  An edit that grows either fails here.  It reads the compiler's report
only.  Parsing and the per-kernel checks: tests/kernel_resources.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_resources as KR  # noqa: E402

TILE = 16
LDS_BYTES = 4 * ((TILE + 3) * 256 + 512 + 4 * 512)
KERNELS = {"gt_yin_f0_kernel": (LDS_BYTES, 2)}


def test_yin_kernel_resources(built):
    from glow_tts_amd import _lib
    assert _lib.lib().gt_yin_tile_frames() == TILE and LDS_BYTES == 29696
    # the file has one kernel; at least two waves per SIMD and two workgroups per CU
    KR.check_kernels("yin_front", KERNELS, max_regs=256, resident=2, at_least=True)
