"""What the tests/test_*_resources.py files share: the parser of the build's per-kernel resource reports
(glow-tts_amd/build/NAME.resources.txt, one line per kernel as build.py writes it from hipcc's kernel-resource-usage remarks) and the
loop that checks a file's kernels against a table.  A plain helper module like tests/gl64.py; the tables, the arithmetic on them and
anything one file checks alone stay in that file."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CU_LDS_BYTES = 160 * 1024


def report_lines(source, only=None):
    """the non-empty lines of the report of csrc/<source>.hip (only: those that contain this text)"""
    with open(os.path.join(ROOT, "glow-tts_amd", "build", source + ".resources.txt")) as f:
        return [l.strip() for l in f if l.strip() and (only is None or only in l)]


def fields(line):
    """one report line -> {field: text}"""
    found = dict(re.findall(r"([A-Za-z][A-Za-z ]*(?:\[[^\]]*\])?)=(\S+)", line.split(None, 1)[1]))
    return {k.strip(): v for k, v in found.items()}


def no_scratch_no_spills(f, line):
    assert f["ScratchSize [bytes/lane]"] == "0", line
    assert f["VGPRs Spill"] == "0" and f["SGPRs Spill"] == "0", line


def check_kernels(source, kernels, max_regs, resident, at_least=False):
    """Every kernel of csrc/<source>.hip is one of `kernels` {name part: (LDS bytes, waves per SIMD)}, each seen once, and has: no
    scratch, no spills, exactly those LDS bytes, that occupancy (at_least: no less), `resident` workgroups' LDS within a CU's 160 KB,
    and VGPRs + AGPRs <= max_regs.  -> {name part: (fields, line)} for what a file checks on top."""
    lines = report_lines(source)
    assert len(lines) == len(kernels), lines
    seen = {}
    for line in lines:
        name = next((k for k in kernels if k in line), None)
        assert name is not None and name not in seen, line
        lds, occupancy = kernels[name]
        f = fields(line)
        no_scratch_no_spills(f, line)
        if at_least:
            assert int(f["Occupancy [waves/SIMD]"]) >= occupancy, line
        else:
            assert f["Occupancy [waves/SIMD]"] == str(occupancy), line
        assert int(f["LDS Size [bytes/block]"]) == lds, line
        assert resident * int(f["LDS Size [bytes/block]"]) <= CU_LDS_BYTES, line
        assert int(f["VGPRs"]) + int(f["AGPRs"]) <= max_regs, line
        seen[name] = (f, line)
    assert set(seen) == set(kernels)
    return seen
