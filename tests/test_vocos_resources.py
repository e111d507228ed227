"""The Vocos kernels (csrc/vocos.hip) as the compiler built them: twelve kernels — gt_vocos_norm for C / 64 = 1..8,
gt_vocos_mlp for C = 128, 256, 512, gt_vocos_polar — none with scratch or spilled registers.  What DESIGN.md 4.25 states:

  gt_vocos_norm   no LDS, at most 128 registers: four waves per SIMD or more at every width
  gt_vocos_mlp    dynamic LDS of gt_vocos_mlp_lds_bytes(C) = 52 224 / 68 608 / 101 376 bytes: 3 / 2 / 1 workgroups a CU within its 160 KB,
                  and the registers (VGPRs + AGPRs) to match — at most 168 / 256 / 512, i.e. 3 / 2 / 1 waves per SIMD
  gt_vocos_polar  33 024 bytes of static LDS ([32][129] floats, twice), at most 64 registers, four workgroups a CU

An edit that grows any of these fails here.  Parsing and the per-kernel checks: tests/kernel_resources.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_resources as KR  # noqa: E402

MLP = {128: (52224, 3, 168), 256: (68608, 2, 256), 512: (101376, 1, 512)}          # C: (dynamic LDS, workgroups a CU = waves per SIMD, registers)


def test_vocos_kernel_resources(built):
    from glow_tts_amd import _lib
    L = _lib.lib()
    kernels = {f"gt_vocos_norm_kernelILi{nc}E": (0, 4) for nc in range(1, 9)}
    kernels.update({f"gt_vocos_mlp_kernelILi{C}E": (0, occ) for C, (_, occ, _) in MLP.items()})     # its LDS is dynamic: checked below
    kernels["gt_vocos_polar_kernel"] = (33024, 4)
    seen = KR.check_kernels("vocos", kernels, max_regs=512, resident=4, at_least=True)
    for name, (f, line) in seen.items():
        assert f["Dynamic Stack"] == "False", line
        regs = int(f["VGPRs"]) + int(f["AGPRs"])
        if "norm" in name:
            assert regs <= 128, line
        elif "polar" in name:
            assert regs <= 64, line
    for C, (lds, resident, max_regs) in MLP.items():
        f, line = seen[f"gt_vocos_mlp_kernelILi{C}E"]
        assert int(f["VGPRs"]) + int(f["AGPRs"]) <= max_regs, line
        assert L.gt_vocos_mlp_lds_bytes(C) == lds and resident * lds <= KR.CU_LDS_BYTES < (resident + 1) * lds
        assert f["Occupancy [waves/SIMD]"] == str(resident), line                  # four waves a workgroup: one per SIMD and workgroup
