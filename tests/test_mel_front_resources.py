"""The mel front end's kernels (csrc/mel_front.hip) as the compiler built them: no scratch, no spilled registers, and the LDS
footprint and occupancy DESIGN.md 4.17 states — ONE buffer of 68 880 bytes per workgroup (the 17 152 samples a 64-frame tile spans, one
pad word per 256, rounded to 16 bytes; the reduction aliases it), two workgroups = two waves per SIMD on a CU's 160 KB, and a
register budget (at most 256) that allows those two waves.  An edit that grows either loses the second resident workgroup and fails here.
Parsing and the per-kernel checks: tests/kernel_resources.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_resources as KR  # noqa: E402

LDS_BYTES = 17220 * 4
KERNELS = {"gt_mel_front_kernelILi3E": (LDS_BYTES, 2), "gt_mel_front_kernelILi4E": (LDS_BYTES, 2), "gt_mel_pack_kernel": (0, 8)}


def test_mel_front_kernels_resources(built):
    span = 63 * 256 + 1024
    assert LDS_BYTES == 68880 and span == 17152 and span + (span >> 8) <= 17220 < span + (span >> 8) + 4
    KR.check_kernels("mel_front", KERNELS, max_regs=256, resident=2)     # every kernel of the file is one of the three
