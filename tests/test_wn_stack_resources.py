"""The whole-WaveNet backward kernel runs two waves per SIMD (512 threads, one workgroup per CU): every instantiation of
gt_wn_stack_bwd_kernel must report occupancy 2, no scratch and no spilled registers in the compiler's resource remarks, so
that an edit which pushes it back over 256 VGPR + AGPR per wave fails here rather than silently halving its occupancy."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "glow-tts_amd", "build", "wn_stack.resources.txt")


def test_wn_stack_backward_runs_two_waves_per_simd(built):
    with open(REPORT) as f:
        lines = [l.strip() for l in f if "gt_wn_stack_bwd_kernel" in l]
    assert len(lines) == 8, lines                    # COND x DROP x (64-row, 32-row form)
    for line in lines:
        fields = dict(re.findall(r"([A-Za-z][A-Za-z ]*(?:\[[^\]]*\])?)=(\S+)", line.split(None, 1)[1]))
        fields = {k.strip(): v for k, v in fields.items()}
        assert fields["Occupancy [waves/SIMD]"] == "2", line
        assert fields["ScratchSize [bytes/lane]"] == "0", line
        assert fields["VGPRs Spill"] == "0", line
        assert int(fields["VGPRs"]) + int(fields["AGPRs"]) <= 256, line
