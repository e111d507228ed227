"""The mel-inversion kernel (csrc/gl_mel.hip) as the compiler built it: no scratch, no spilled registers, and the LDS footprint and
occupancy DESIGN.md 4.21 states — expf(mel) of 32 frames at the largest n_mel, 128 x 32 words, and 32 rows of mel_pinv at a pitch of
129 words: 16 384 + 16 512 = 32 896 bytes, four workgroups = four waves per SIMD on a CU's 160 KB.  Same parsing as
tests/test_griffin_lim_resources.py."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "glow-tts_amd", "build", "gl_mel.resources.txt")
LDS_BYTES = (128 * 32 + 32 * 129) * 4
KERNELS = {"gt_gl_from_mel_kernel": (LDS_BYTES, 4)}


def _fields(line):
    fields = dict(re.findall(r"([A-Za-z][A-Za-z ]*(?:\[[^\]]*\])?)=(\S+)", line.split(None, 1)[1]))
    return {k.strip(): v for k, v in fields.items()}


def test_gl_mel_kernel_resources(built):
    assert LDS_BYTES == 32896
    with open(REPORT) as f:
        lines = [l.strip() for l in f if l.strip()]
    assert len(lines) == len(KERNELS), lines                 # the file holds the one kernel
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
        assert occupancy * int(fields["LDS Size [bytes/block]"]) <= 160 * 1024 < (occupancy + 1) * int(fields["LDS Size [bytes/block]"]), line
        assert int(fields["VGPRs"]) + int(fields["AGPRs"]) <= 128, line      # four waves per SIMD of 512 registers
    assert seen == set(KERNELS)
