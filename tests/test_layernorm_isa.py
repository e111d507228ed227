"""The LayerNorm kernels (csrc/encoder_ops.hip) as compiled for gfx950: every load of a wave's rows is issued before the first use
(DESIGN.md 4.10 (5)).  What keeps the compiler from sinking loads into the blocks that use them is a scheduling hint (`ln_landed`, an
empty asm statement naming every loaded register), which nothing in the language pins, so the compiled code is read here: in each
of the 3 forward and 2 x 9 backward instantiations no global load follows the first `s_waitcnt vmcnt`, and the waits end in ONE
`vmcnt(0)` (the parent's backward had 25 of them, one per operand).  Compiles the one source file to assembly; needs no GPU."""
import importlib.util
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layernorm_kernels_issue_every_load_before_the_first_wait(tmp_path):
    spec = importlib.util.spec_from_file_location("_gt_build_flags", os.path.join(ROOT, "glow-tts_amd", "build.py"))
    B = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(B)
    out = str(tmp_path / "encoder_ops.s")
    flags = [f for f in B.FLAGS if not f.startswith("-Rpass") and f != "-fPIC"]
    subprocess.check_call([B.HIPCC, *flags, "-S", "--cuda-device-only", os.path.join(B.CSRC, "encoder_ops.hip"), "-o", out],
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    with open(out) as f:
        text = f.read()
    names = re.findall(r"^(_ZN\S*gt_layernorm_(?:fwd|bwd)_kernelI\S*):\s*(?:;.*)?$", text, re.M)
    assert len(names) == 3 + 2 * 9, names
    for n in names:
        i = text.index("\n" + n + ":")
        body = text[i:text.index("s_endpgm", i)]
        ops = re.findall(r"^\s+(global_load_\w+|s_waitcnt [^;\n]*vmcnt\(\d+\))", body, re.M)
        first_wait = next(k for k, o in enumerate(ops) if o.startswith("s_waitcnt"))
        late = [o for o in ops[first_wait:] if o.startswith("global_load")]
        zero = sum("vmcnt(0)" in o for o in ops)
        print(f"{n}: {first_wait} loads, {len(ops) - first_wait - len(late)} waits, {zero} vmcnt(0), {len(late)} loads behind a wait")
        assert not late, n
        assert zero == 1, n
