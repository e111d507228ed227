"""The mel front end's kernels (csrc/mel_front.hip) as the compiler built them: no scratch, no spilled registers, and the LDS
footprint and occupancy DESIGN.md 4.17 states — ONE buffer of 68 880 bytes per workgroup (the 17 152 samples a 64-frame tile spans, one
pad word per 256, rounded to 16 bytes; the reduction aliases it), two workgroups = two waves per SIMD on a CU's 160 KB, and a
register budget (at most 256) that allows those two waves.  An edit that grows either loses the second resident workgroup and fails here.
Same parsing as tests/test_dds_layer_resources.py."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "glow-tts_amd", "build", "mel_front.resources.txt")
LDS_BYTES = 17220 * 4
KERNELS = {"gt_mel_front_kernelILi3E": (LDS_BYTES, 2), "gt_mel_front_kernelILi4E": (LDS_BYTES, 2), "gt_mel_pack_kernel": (0, 8)}


def _fields(line):
    fields = dict(re.findall(r"([A-Za-z][A-Za-z ]*(?:\[[^\]]*\])?)=(\S+)", line.split(None, 1)[1]))
    return {k.strip(): v for k, v in fields.items()}


def test_mel_front_kernels_resources(built):
    span = 63 * 256 + 1024
    assert LDS_BYTES == 68880 and span == 17152 and span + (span >> 8) <= 17220 < span + (span >> 8) + 4
    with open(REPORT) as f:
        lines = [l.strip() for l in f if l.strip()]
    assert len(lines) == len(KERNELS), lines                 # every kernel of the file is one of the three
    seen = set()
    for line in lines:
        name = next((k for k in KERNELS if k in line), None)
        assert name is not None and name not in seen, line
        seen.add(name)
        lds, occupancy = KERNELS[name]
        fields = _fields(line)
        assert fields["ScratchSize [bytes/lane]"] == "0", line
        assert fields["VGPRs Spill"] == "0" and fields["SGPRs Spill"] == "0", line
        assert fields["Occupancy [waves/SIMD]"] == str(occupancy), line
        assert int(fields["LDS Size [bytes/block]"]) == lds, line
        assert 2 * int(fields["LDS Size [bytes/block]"]) <= 160 * 1024, line
        assert int(fields["VGPRs"]) + int(fields["AGPRs"]) <= 256, line
    assert seen == set(KERNELS)
