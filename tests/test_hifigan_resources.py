"""The vocoder kernel's six instantiations (csrc/hifigan.hip: positions x channels tile 128 x 128 / 128 x 64 / 128 x 32, each with a
64- or a 32-channel Cin chunk) as the compiler built them: no scratch, no spilled registers, no static LDS — the LDS is dynamic,
(128 + (taps - 1) dil) (2 chunk + 16) bytes as DESIGN.md 4.23 states, at most 64 KB — and registers that allow the waves per SIMD stated
here: 5 for the widest tile (four accumulators per wave, <= 96 registers), 8 for the other two (<= 64).  The widest halo of the
generator (taps 11, dil 5) takes 25 632 bytes at the 64-channel chunk: six workgroups on a CU's 160 KB.  An edit that grows any of these
fails here.  Parsing and the per-kernel checks: tests/kernel_resources.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_resources as KR  # noqa: E402

# template arguments <waves along the positions, row tiles per wave, column tiles per wave, k-steps per chunk> as they appear in the mangled name
WIDE = {"ILi1ELi4ELi1ELi4EE": (0, 5), "ILi1ELi4ELi1ELi2EE": (0, 5)}
NARROW = {"ILi2ELi2ELi1ELi4EE": (0, 8), "ILi2ELi2ELi1ELi2EE": (0, 8), "ILi4ELi1ELi1ELi4EE": (0, 8), "ILi4ELi1ELi1ELi2EE": (0, 8)}


def test_hifigan_kernel_resources(built):
    from glow_tts_amd import _lib
    L = _lib.lib()
    seen = KR.check_kernels("hifigan", {**WIDE, **NARROW}, max_regs=96, resident=1)
    for name, (f, line) in seen.items():
        assert "gt_voc_conv_kernel" in line and f["Dynamic Stack"] == "False", line
        if name in NARROW:
            assert int(f["VGPRs"]) + int(f["AGPRs"]) <= 64, line
    lds = L.gt_voc_lds_bytes(512, 11, 5)
    assert lds == (128 + 50) * 144 == 25632 and KR.CU_LDS_BYTES // lds == 6
    assert L.gt_voc_lds_bytes(32, 3, 1) == 130 * 80 and KR.CU_LDS_BYTES // (130 * 80) >= 8
