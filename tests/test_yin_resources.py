"""The pitch front end's kernel (csrc/yin_front.hip) as the compiler built it: no scratch, no spilled registers, and the LDS footprint
and occupancy DESIGN.md 4.18 states — the samples a 16-frame tile reads ((16 + 3) * 256 + 512 floats) plus a ring of four frames'
difference functions (4 * 512 floats) = 29 696 bytes per workgroup of two waves, so that five workgroups (at least two) are resident
on a CU's 160 KB, within a register budget (at most 256) that allows them.  An edit that grows either fails here.  It reads the compiler's report
only.  Same parsing as tests/test_mel_front_resources.py."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "glow-tts_amd", "build", "yin_front.resources.txt")
TILE = 16
LDS_BYTES = 4 * ((TILE + 3) * 256 + 512 + 4 * 512)
KERNELS = {"gt_yin_f0_kernel": (LDS_BYTES, 2)}


def _fields(line):
    fields = dict(re.findall(r"([A-Za-z][A-Za-z ]*(?:\[[^\]]*\])?)=(\S+)", line.split(None, 1)[1]))
    return {k.strip(): v for k, v in fields.items()}


def test_yin_kernel_resources(built):
    from glow_tts_amd import _lib
    assert _lib.lib().gt_yin_tile_frames() == TILE and LDS_BYTES == 29696
    with open(REPORT) as f:
        lines = [l.strip() for l in f if l.strip()]
    assert len(lines) == len(KERNELS), lines                 # the file has one kernel
    seen = set()
    for line in lines:
        name = next((k for k in KERNELS if k in line), None)
        assert name is not None and name not in seen, line
        seen.add(name)
        lds, waves = KERNELS[name]
        fields = _fields(line)
        assert fields["ScratchSize [bytes/lane]"] == "0", line
        assert fields["VGPRs Spill"] == "0" and fields["SGPRs Spill"] == "0", line
        assert int(fields["Occupancy [waves/SIMD]"]) >= waves, line
        assert int(fields["LDS Size [bytes/block]"]) == lds, line
        assert 2 * int(fields["LDS Size [bytes/block]"]) <= 160 * 1024, line          # at least two workgroups per CU
        assert int(fields["VGPRs"]) + int(fields["AGPRs"]) <= 256, line
    assert seen == set(KERNELS)
