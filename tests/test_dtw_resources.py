"""The synthesis metrics' kernels (csrc/dtw.hip) as the compiler built them: no scratch, no spilled registers, and what DESIGN.md
4.27 states — the DTW kernel keeps all its LDS dynamic (no static bytes in front of the 16-byte aligned image of b's features) and
its registers allow the four waves per SIMD that a workgroup of sixteen waves needs (at most 128 VGPRs); the cepstrum kernel holds
the [n][16] matrix in 8 192 static bytes, the F0 kernel its five reduction rows in 5 120, the path kernel one word, all three at eight waves per SIMD.  The dynamic
footprint of gt_dtw_f32 is gt_dtw_lds_bytes: 512 bytes of ring per wave, the pass row past 1 024 rows, and 64 bytes per column
of b where all of it fits a CU's 160 KB — 55 296 bytes for the bench shape (800 x 760), where two workgroups of 13 waves fit a CU.
Parsing and the per-kernel checks: tests/kernel_resources.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_resources as KR  # noqa: E402

KERNELS = {"gt_mel_cepstrum_kernel": (8192, 8), "gt_dtw_f0_stats_kernel": (5120, 8), "gt_dtw_path_kernel": (4, 8), "gt_dtw_kernelILb0E": (0, 4),
           "gt_dtw_kernelILb1E": (0, 4)}


def test_dtw_kernel_resources(built):
    from glow_tts_amd import _lib
    L = _lib.lib()
    seen = KR.check_kernels("dtw", KERNELS, max_regs=128, resident=1, at_least=True)
    for name, (f, line) in seen.items():
        assert f["Dynamic Stack"] == "False", line
        if not name.startswith("gt_dtw_kernel"):
            assert int(f["VGPRs"]) + int(f["AGPRs"]) <= 64, line                    # eight waves per SIMD
    bench = L.gt_dtw_lds_bytes(800, 760)
    assert bench == 13 * 512 + 64 * 760 and KR.CU_LDS_BYTES // bench == 2 and 2 * 13 <= 32
    for Fa, Fb in ((1, 1), (1024, 2432), (4096, 4096), (64, 4096), (4096, 64)):     # every supported shape fits one CU
        assert 0 < L.gt_dtw_lds_bytes(Fa, Fb) <= KR.CU_LDS_BYTES, (Fa, Fb)
