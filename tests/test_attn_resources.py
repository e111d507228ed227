"""The fifteen MFMA attention kernels (csrc/attn_mfma.hip, csrc/attn_long.hip) as the compiler built them, against what they had
before their tile steps moved into csrc/attn_frag.h (profiles/attn_parts_isa.txt): no scratch, no spilled vector registers, the same
occupancy, the same static LDS bytes (the dynamic part is the launch's and is not in the report), and VGPRs + AGPRs within that
occupancy's class — a register more or less passes, a lost wave does not.  Three of them have no room to give:
gt_attn_long_bwd_q_stats_kernel (252 of 256 at two waves before), gt_attn_long_bwd_kv_stats_kernel and gt_attn_fwd_mfma_kernel<8>
(all 256 VGPRs plus AGPRs at one).
"No spills" is read here, on purpose, as: no scratch, no spilled vector register, and no more scalar registers parked in vector
lanes ("SGPRs Spill": no memory behind them) than the kernel had before the move.  Three kernels already had such parked registers
(gt_attn_fwd_mfma_kernel<5> 250, <8> 442, gt_attn_long_bwd_kv_stats_kernel 20), so zero would fail on the unchanged code; their
earlier counts are the bound, and every other kernel's bound is zero.
The report's parser: tests/kernel_resources.py (its check_kernels takes one register bound per file and no scalar spill at all,
so the loop is here)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_resources as KR  # noqa: E402

REGS_AT = {1: 512, 2: 256, 3: 168, 4: 128}          # VGPRs + AGPRs a wave may hold at that many waves per SIMD

# name part: (static LDS bytes, waves per SIMD, scalar registers parked in vector lanes at most)
MFMA = {"gt_attn_fwd_mfma_kernelILi5E": (0, 1, 250), "gt_attn_fwd_mfma_kernelILi8E": (0, 1, 442), "gt_attn_fwd_mfma_long_kernelILi12E": (0, 2, 0),
        "gt_attn_bwd_q_mfma_kernelILi8ELi2E": (0, 3, 0), "gt_attn_bwd_q_mfma_kernelILi12ELi4E": (0, 3, 0),
        "gt_attn_bwd_kv_mfma_kernelILi8E": (0, 3, 0), "gt_attn_bwd_kv_mfma_kernelILi12E": (0, 4, 0), "gt_attn_bwd_fused_kernel": (0, 2, 0)}
LONG = {"gt_attn_long_fwd_kernelILb1E": (30720, 2, 0), "gt_attn_long_fwd_kernelILb0E": (30720, 2, 0), "gt_attn_long_fwd_stats_kernel": (30720, 2, 0),
        "gt_attn_long_bwd_q_kernel": (0, 2, 0), "gt_attn_long_bwd_q_stats_kernel": (0, 2, 0),
        "gt_attn_long_bwd_kv_kernel": (24576, 2, 0), "gt_attn_long_bwd_kv_stats_kernel": (25344, 1, 20)}


def _check(source, kernels):
    lines = KR.report_lines(source)
    assert len(lines) == len(kernels), lines
    seen = set()
    for line in lines:
        name = next((k for k in kernels if k in line), None)
        assert name is not None and name not in seen, line
        seen.add(name)
        lds, occupancy, parked = kernels[name]
        f = KR.fields(line)
        assert f["ScratchSize [bytes/lane]"] == "0" and f["VGPRs Spill"] == "0" and f["Dynamic Stack"] == "False", line
        assert int(f["SGPRs Spill"]) <= parked, line
        assert f["Occupancy [waves/SIMD]"] == str(occupancy), line
        assert int(f["LDS Size [bytes/block]"]) == lds, line
        assert int(f["VGPRs"]) <= 256 and int(f["VGPRs"]) + int(f["AGPRs"]) <= REGS_AT[occupancy], line
    assert seen == set(kernels)


def test_attn_mfma_kernel_resources(built):
    _check("attn_mfma", MFMA)


def test_attn_long_kernel_resources(built):
    _check("attn_long", LONG)
