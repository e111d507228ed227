"""The denoiser's analysis kernel (csrc/denoise.hip) as the compiler built it: no scratch, no spilled registers, the folded-DFT tile's
68 880-byte sample buffer as its only LDS (gt_gl_project's), two workgroups = two waves per SIMD on a CU's 160 KB, in a register
budget (at most 256) that allows them.  Parsing and the per-kernel checks: tests/kernel_resources.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_resources as KR  # noqa: E402

SAMPLE_LDS = 17220 * 4


def test_denoise_kernel_resources(built):
    assert SAMPLE_LDS == 68880
    KR.check_kernels("denoise", {"gt_denoise_spec_kernel": (SAMPLE_LDS, 2)}, max_regs=256, resident=2)   # the file's one kernel
