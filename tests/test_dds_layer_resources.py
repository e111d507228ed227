"""The fused DDSConv layer kernels (csrc/dds_layer.hip) as the compiler built them: no scratch, no spilled registers, and the
occupancy and LDS footprint DESIGN.md 4.6.1 states — ONE 64-row tile of 50 176 bytes (the bf16 hi / lo operand rows, then the fp32
product, at the same 784-byte pitch; the backward adds the 1 KB fold buffer of its parameter gradients), three workgroups = three
waves per SIMD on a CU's 160 KB, and a register budget (VGPR + AGPR <= 168) that allows those three waves.  An edit that grows the
tile or the registers fails here rather than silently losing a resident workgroup.  Parsing and the per-kernel checks: tests/kernel_resources.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_resources as KR  # noqa: E402

TILE_BYTES = 64 * (2 * 192 + 8) * 2
LDS = {"gt_dds_layer_fwd_kernel": TILE_BYTES, "gt_dds_layer_bwd_kernel": TILE_BYTES + 256 * 4}


def test_dds_layer_kernels_resources(built):
    assert TILE_BYTES == 50176 == 64 * (192 + 4) * 4
    assert len(LDS) == 2                                # every kernel of the file is one of the two
    KR.check_kernels("dds_layer", {name: (lds, 3) for name, lds in LDS.items()}, max_regs=168, resident=3)
