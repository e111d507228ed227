"""The activation kernel (csrc/voc_snake.hip) as the compiler built it: one kernel, no scratch, no spilled registers,
no LDS, and at most 96 registers — five waves per SIMD, what its two loads in flight per thread are sized for (four channels per
thread took 169 registers and two waves).  An edit that grows any of these fails here.  Parsing and the per-kernel checks:
tests/kernel_resources.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_resources as KR  # noqa: E402


def test_voc_snake_kernel_resources(built):
    seen = KR.check_kernels("voc_snake", {"gt_voc_snake_kernel": (0, 5)}, max_regs=96, resident=1, at_least=True)
    f, line = seen["gt_voc_snake_kernel"]
    assert f["Dynamic Stack"] == "False" and f["ScratchSize [bytes/lane]"] == "0", line
