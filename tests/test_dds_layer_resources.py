"""The fused DDSConv layer kernels (csrc/dds_layer.hip) as the compiler built them: no scratch, no spilled registers, and the
occupancy and LDS footprint DESIGN.md 4.6.1 states — ONE 64-row tile of 50 176 bytes (the bf16 hi / lo operand rows, then the fp32
product, at the same 784-byte pitch; the backward adds the 1 KB fold buffer of its parameter gradients), three workgroups = three
waves per SIMD on a CU's 160 KB, and a register budget (VGPR + AGPR <= 168) that allows those three waves.  An edit that grows the
tile or the registers fails here rather than silently losing a resident workgroup.  Same parsing as tests/test_wn_stack_resources.py."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "glow-tts_amd", "build", "dds_layer.resources.txt")
TILE_BYTES = 64 * (2 * 192 + 8) * 2
LDS = {"gt_dds_layer_fwd_kernel": TILE_BYTES, "gt_dds_layer_bwd_kernel": TILE_BYTES + 256 * 4}


def _fields(line):
    fields = dict(re.findall(r"([A-Za-z][A-Za-z ]*(?:\[[^\]]*\])?)=(\S+)", line.split(None, 1)[1]))
    return {k.strip(): v for k, v in fields.items()}


def test_dds_layer_kernels_resources(built):
    assert TILE_BYTES == 50176 == 64 * (192 + 4) * 4
    with open(REPORT) as f:
        lines = [l.strip() for l in f if l.strip()]
    assert len(lines) == 2, lines                      # every kernel of the file is one of the two
    seen = set()
    for line in lines:
        name = next((k for k in LDS if k in line), None)
        assert name is not None and name not in seen, line
        seen.add(name)
        fields = _fields(line)
        assert fields["ScratchSize [bytes/lane]"] == "0", line
        assert fields["VGPRs Spill"] == "0" and fields["SGPRs Spill"] == "0", line
        assert fields["Occupancy [waves/SIMD]"] == "3", line
        assert int(fields["LDS Size [bytes/block]"]) == LDS[name], line
        assert 3 * int(fields["LDS Size [bytes/block]"]) <= 160 * 1024, line
        assert int(fields["VGPRs"]) + int(fields["AGPRs"]) <= 168, line
    assert seen == set(LDS)
