"""The loudness kernels (csrc/loudness.hip) as the compiler built them: no scratch, no spilled registers, and the stated LDS — the two
chunk passes stage 256 chunks of up to 50 samples at a pitch of 51 words (52 224 bytes: three workgroups on a CU's 160 KB), the state
scan holds 256 run states, 16 group states and the carry in double (8 736 bytes; its thread keeps a run's 16 end states in registers, two waves per SIMD:
one workgroup per utterance, occupancy is not what it waits for), the gate kernel one double and one float per thread (3 072 bytes),
the scale pass none.  Parsing and the per-kernel checks: tests/kernel_resources.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_resources as KR  # noqa: E402

CHUNK_LDS = 256 * 51 * 4
SCAN_LDS = 256 * 4 * 8 + 16 * 4 * 8 + 4 * 8
GATE_LDS = 256 * 8 + 256 * 4


def test_loudness_kernel_resources(built):
    assert (CHUNK_LDS, SCAN_LDS, GATE_LDS) == (52224, 8736, 3072)
    KR.check_kernels("loudness", {"gt_loud_chunk_kernelILb0": (CHUNK_LDS, 3), "gt_loud_chunk_kernelILb1": (CHUNK_LDS, 3),
                                  "gt_loud_scan_kernel": (SCAN_LDS, 2), "gt_loud_gate_kernel": (GATE_LDS, 8),
                                  "gt_loud_apply_kernel": (0, 8)}, max_regs=256, resident=3)
