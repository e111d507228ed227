"""The LayerNorm kernels (csrc/encoder_ops.hip) as the compiler built them: one forward per (a, y) presence and one backward per
(geometry, a, y, dout_f32, dout_bf16) presence — 3 + 2 x 9 instantiations —, none with scratch or spilled registers, the forward
without LDS, the backward with its fold buffer of 2 x waves x 256 floats (32 KB at 16 waves, 8 KB at 4), and registers that leave the
residency DESIGN.md 4.10 (5) states: a 16-wave workgroup is resident only as a whole, so its kernels must allow at least 4 waves per
SIMD (at most 128 registers); the 4-wave x 4-row form holds the loads of four rows in at most 140 VGPRs, which still is 3 waves per SIMD.  The ceilings are asserted as register counts, so growth shows before it costs a whole occupancy step.  Parsing:
tests/kernel_resources.py; the checks are this file's own (instantiations told apart by their template arguments)."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_resources as KR  # noqa: E402

GEOMETRIES = {(16, 2), (4, 4)}        # (waves, rows per wave): the atomics form from 2048 rows on; the partials form and the atomics form below


def test_layernorm_kernels_resources(built):
    lines = KR.report_lines("encoder_ops", only="gt_layernorm_")
    fwd, bwd = set(), set()
    for line in lines:
        name = line.split()[0]
        fields = KR.fields(line)
        KR.no_scratch_no_spills(fields, line)
        occ, lds = int(fields["Occupancy [waves/SIMD]"]), int(fields["LDS Size [bytes/block]"])
        m = re.search(r"gt_layernorm_fwd_kernelILb([01])ELb([01])E", name)
        if m:
            fwd.add(m.groups())
            assert lds == 0 and occ >= 4, line
            continue
        m = re.search(r"gt_layernorm_bwd_kernelILi(\d+)ELi(\d+)ELb([01])ELb([01])ELb([01])ELb([01])E", name)
        assert m, line
        waves, rows = int(m.group(1)), int(m.group(2))
        assert (waves, rows) in GEOMETRIES, line
        bwd.add((waves, rows) + m.groups()[2:])
        assert lds == 2 * waves * 256 * 4, line
        regs = int(fields["VGPRs"]) + int(fields.get("AGPRs", 0))
        if waves == 16:
            assert regs <= 128 and occ >= 4, line
        else:
            assert regs <= 140 and occ >= 3, line
    pairs = {("1", "0"), ("0", "1"), ("1", "1")}
    assert fwd == pairs
    assert bwd == {g + ay + dd for g in GEOMETRIES for ay in pairs for dd in pairs}
