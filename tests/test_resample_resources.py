"""The resampler's kernel (csrc/resample.hip) as the compiler built it: no scratch, no spilled registers, no static LDS — its LDS is
dynamic, sized per rate pair by the host — and registers that allow the eight waves per SIMD the compiler reports.  The dynamic
footprint is what DESIGN.md 4.22 states: 4 (round4(up (T | 1)) + round4((up - 1 + 511 down) div up + T)) bytes, at most 64 KB, i.e.
for the six pairs of the issue 31 104, 38 624, 4 432, 15 856, 40 064 and 57 776 bytes = 5, 4, 36, 10, 4 and 2 workgroups of four
waves on a CU's 160 KB (at most 8 fit its wave slots).  An edit that grows any of these fails here.  It reads the compiler's report
and asks the library for the sizes.  Parsing and the per-kernel checks: tests/kernel_resources.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_resources as KR  # noqa: E402
import resample64 as R  # noqa: E402

KERNELS = {"gt_resample_kernel": (0, 8)}
LDS = {(48000, 22050): (31104, 5), (16000, 22050): (38624, 4), (44100, 22050): (4432, 36), (24000, 22050): (15856, 10),
       (22050, 16000): (40064, 4), (32000, 22050): (57776, 2)}


def test_resample_kernel_resources(built):
    from glow_tts_amd import _lib
    L = _lib.lib()
    seen = KR.check_kernels("resample", KERNELS, max_regs=64, resident=8)
    f, line = seen["gt_resample_kernel"]
    assert f["Dynamic Stack"] == "False", line
    for pair, (lds, resident) in LDS.items():
        up, down = R.ratio(*pair)
        assert L.gt_resample_lds_bytes(up, down) == lds, pair
        assert KR.CU_LDS_BYTES // lds == resident and resident >= 2, pair
