"""The mel-inversion kernel (csrc/gl_mel.hip) as the compiler built it: no scratch, no spilled registers, and the LDS footprint and
occupancy DESIGN.md 4.21 states — expf(mel) of 32 frames at the largest n_mel, 128 x 32 words, and 32 rows of mel_pinv at a pitch of
129 words: 16 384 + 16 512 = 32 896 bytes, four workgroups = four waves per SIMD on a CU's 160 KB.  Parsing and the
per-kernel checks: tests/kernel_resources.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_resources as KR  # noqa: E402

LDS_BYTES = (128 * 32 + 32 * 129) * 4
KERNELS = {"gt_gl_from_mel_kernel": (LDS_BYTES, 4)}


def test_gl_mel_kernel_resources(built):
    assert LDS_BYTES == 32896
    # the file holds the one kernel; four waves per SIMD of 512 registers, four workgroups' LDS on a CU and not five
    seen = KR.check_kernels("gl_mel", KERNELS, max_regs=128, resident=4)
    for name, (f, line) in seen.items():
        assert KR.CU_LDS_BYTES < (KERNELS[name][1] + 1) * int(f["LDS Size [bytes/block]"]), line
