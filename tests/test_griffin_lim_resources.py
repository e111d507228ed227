"""The waveform back end's kernels (csrc/griffin_lim.hip) as the compiler built them: no scratch, no spilled registers, and the LDS
footprint and occupancy DESIGN.md 4.20 states — gt_gl_project the mel front end's 68 880-byte sample buffer, gt_istft one pass buffer
of 4 waves x (plain | mirror) x 32 rows x 65 words = 66 560 bytes, two workgroups = two waves per SIMD each on a CU's 160 KB, in a
register budget (at most 256) that allows them; the two elementwise kernels no LDS and full occupancy.  Parsing and the
per-kernel checks: tests/kernel_resources.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_resources as KR  # noqa: E402

PROJECT_LDS, ISTFT_LDS = 17220 * 4, 4 * 2 * 32 * 65 * 4
KERNELS = {"gt_gl_pack_kernel": (0, 8), "gt_gl_polar_kernel": (0, 8), "gt_gl_project_kernel": (PROJECT_LDS, 2),
           "gt_istft_kernel": (ISTFT_LDS, 2)}


def test_griffin_lim_kernels_resources(built):
    assert PROJECT_LDS == 68880 and ISTFT_LDS == 66560
    KR.check_kernels("griffin_lim", KERNELS, max_regs=256, resident=2)   # every kernel of the file is one of the four
