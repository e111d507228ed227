"""The between-WaveNet kernels (csrc/wn_boundary.hip) and the five-launch flow kernels (csrc/flow_ops.hip) return, bit for bit, what
they returned before their row maths moved into csrc/flow_rows.h and the boundary kernels' tile steps became shared:
tools/wn_boundary_trace.py's passes (the three layouts of tests/test_wn_boundary_fp64_gpu.py, sigmoid_scale off and on, every launch
of train forward + backward on both parameter-gradient routes and of eval reverse, the folded squeeze / unsqueeze forms, the six
five-launch kernels on the recorded operands) run again, and the sha256 of every tensor with one writer per element is compared with
the listing recorded at the parent commit (profiles/wn_boundary_parts_trace_parent.txt).  The log-dets and the parameter gradients are
atomic sums whose bits depend on arrival order; the float64 tests bound them."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_boundary_bits_match_the_recorded_listing(built):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import wn_boundary_trace
    with open(os.path.join(ROOT, "profiles", "wn_boundary_parts_trace_parent.txt")) as f:
        want = [l.rstrip("\n") for l in f if l.strip() and not l.startswith("#")]
    got = [l for lines, _, _ in wn_boundary_trace.listing() for l in lines]
    # per pass: forward 4 + 6 + 6 + 3 tensors, backward 4 + 2 (5 + 4) + (2 + 1), reverse 2 + 2 + 2 + 1, five-launch 9; on rows (no folded
    # squeeze) the first forward and reverse launches write one tensor less
    assert len(want) == sum(60 if wn_boundary_trace.LAYOUTS[layout][2] else 58 for layout, _ in wn_boundary_trace.PASSES)
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want)
