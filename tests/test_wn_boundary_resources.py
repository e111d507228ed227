"""The nine between-WaveNet kernels and gt_boundary_param_reduce_kernel (csrc/wn_boundary.hip) as the compiler built them, against what
they had before their tile steps became shared and their row maths moved into csrc/flow_rows.h (profiles/wn_boundary_parts_isa.txt):
no scratch, no spilled vector register, no scalar register parked in vector lanes, no static LDS (the tiles are the launch's dynamic
LDS and are not in the report), the parent's occupancy, and VGPRs + AGPRs within that occupancy's class — a register more or less
passes, a lost wave does not.  gt_wn_boundary_bwd_kernel<false, true> has the least room: 201 + 48 of 256 at two waves before.
The six five-launch kernels of csrc/flow_ops.hip that share those row maths: no scratch, no spills, occupancy no lower than before,
the same static LDS.  The report's parser: tests/kernel_resources.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_resources as KR  # noqa: E402

REGS_AT = {1: 512, 2: 256, 3: 168, 4: 128, 8: 64}   # VGPRs + AGPRs a wave may hold at that many waves per SIMD

# name part: waves per SIMD at the parent commit (its VGPRs + AGPRs beside it)
BOUNDARY = {"gt_boundary_param_reduce_kernel": 8,                                      # 20 + 0
            "gt_wn_boundary_fwd_kernelILb1ELb1E": 1, "gt_wn_boundary_fwd_kernelILb1ELb0E": 1, "gt_wn_boundary_fwd_kernelILb0ELb1E": 2,   # 256 + 52, 256 + 51, 124 + 48
            "gt_wn_boundary_rev_kernelILb1ELb1E": 1, "gt_wn_boundary_rev_kernelILb1ELb0E": 1, "gt_wn_boundary_rev_kernelILb0ELb1E": 3,   # 252 + 48, 226 + 48, 90 + 48
            "gt_wn_boundary_bwd_kernelILb1ELb1E": 1, "gt_wn_boundary_bwd_kernelILb1ELb0E": 1, "gt_wn_boundary_bwd_kernelILb0ELb1E": 2}   # 256 + 58, 256 + 42, 201 + 48
# name part: (static LDS bytes, waves per SIMD at the parent commit)
FIVE_LAUNCH = {"gt_coupling_fwd_kernel": (16, 8), "gt_coupling_rev_kernel": (0, 8), "gt_coupling_bwd_kernel": (0, 8),
               "gt_actnorm_invconv_fwd_kernel": (0, 8), "gt_actnorm_invconv_rev_kernel": (0, 8), "gt_actnorm_invconv_bwd_kernel": (8464, 7)}


def test_wn_boundary_kernel_resources(built):
    lines = KR.report_lines("wn_boundary")
    assert len(lines) == len(BOUNDARY), lines
    seen = set()
    for line in lines:
        name = next((k for k in BOUNDARY if k in line), None)
        assert name is not None and name not in seen, line
        seen.add(name)
        occupancy = BOUNDARY[name]
        f = KR.fields(line)
        KR.no_scratch_no_spills(f, line)
        assert f["Dynamic Stack"] == "False" and int(f["LDS Size [bytes/block]"]) == 0, line
        assert f["Occupancy [waves/SIMD]"] == str(occupancy), line
        assert int(f["VGPRs"]) <= 256 and int(f["VGPRs"]) + int(f["AGPRs"]) <= REGS_AT[occupancy], line
    assert seen == set(BOUNDARY)


def test_five_launch_flow_kernel_resources(built):
    seen = set()
    for line in KR.report_lines("flow_ops"):
        name = next((k for k in FIVE_LAUNCH if k in line), None)
        if name is None:
            continue
        assert name not in seen, line
        seen.add(name)
        lds, occupancy = FIVE_LAUNCH[name]
        f = KR.fields(line)
        KR.no_scratch_no_spills(f, line)
        assert int(f["Occupancy [waves/SIMD]"]) >= occupancy, line
        assert int(f["LDS Size [bytes/block]"]) == lds, line
    assert seen == set(FIVE_LAUNCH)
