"""The MFMA attention kernels return, bit for bit, what they returned before their tile steps moved into csrc/attn_frag.h:
tools/attn_trace.py's cases (every path of csrc/attn_mfma.hip and csrc/attn_long.hip at the smallest T that reaches each of its
edges, ragged with dropout and uniform without) run again, and the sha256 of every tensor one lane writes — out, P, the row
statistics, both backward workspaces, dq, dk, dv — is compared with the listing recorded at the parent commit
(profiles/attn_parts_trace_parent.txt).  dEk / dEv are atomic sums whose bits depend on arrival order; the float64 tests bound them."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_attention_bits_match_the_recorded_listing(built):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import attn_trace
    with open(os.path.join(ROOT, "profiles", "attn_parts_trace_parent.txt")) as f:
        want = [l.rstrip("\n") for l in f if l.strip() and not l.startswith("#")]
    got = [l for lines, _, _ in attn_trace.listing() for l in lines]
    assert len(want) == sum(6 + 7 * (T > 505) for T, _ in attn_trace.CASES)
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want)
