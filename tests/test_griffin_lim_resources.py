"""The waveform back end's kernels (csrc/griffin_lim.hip) as the compiler built them: no scratch, no spilled registers, and the LDS
footprint and occupancy DESIGN.md 4.20 states — gt_gl_project the mel front end's 68 880-byte sample buffer, gt_istft one pass buffer
of 4 waves x (plain | mirror) x 32 rows x 65 words = 66 560 bytes, two workgroups = two waves per SIMD each on a CU's 160 KB, in a
register budget (at most 256) that allows them; the two elementwise kernels no LDS and full occupancy.  Same parsing as
tests/test_mel_front_resources.py."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "glow-tts_amd", "build", "griffin_lim.resources.txt")
PROJECT_LDS, ISTFT_LDS = 17220 * 4, 4 * 2 * 32 * 65 * 4
KERNELS = {"gt_gl_pack_kernel": (0, 8), "gt_gl_polar_kernel": (0, 8), "gt_gl_project_kernel": (PROJECT_LDS, 2),
           "gt_istft_kernel": (ISTFT_LDS, 2)}


def _fields(line):
    fields = dict(re.findall(r"([A-Za-z][A-Za-z ]*(?:\[[^\]]*\])?)=(\S+)", line.split(None, 1)[1]))
    return {k.strip(): v for k, v in fields.items()}


def test_griffin_lim_kernels_resources(built):
    assert PROJECT_LDS == 68880 and ISTFT_LDS == 66560
    with open(REPORT) as f:
        lines = [l.strip() for l in f if l.strip()]
    assert len(lines) == len(KERNELS), lines                 # every kernel of the file is one of the four
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
