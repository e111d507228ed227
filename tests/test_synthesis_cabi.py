"""CPU tests of the synthesis entry's C-ABI: gt_wn_boundary_rev / gt_boundary_rev_args (the reverse-direction kernel between two
WaveNets, csrc/wn_boundary.hip) are declared, exported, mirrored by the binding with the C struct's size, and validate their
arguments before any launch (no device needed)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_text():
    txt = open(os.path.join(ROOT, "include", "glowtts_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_header_declares_the_reverse_boundary_entry():
    txt = header_text()
    assert re.search(r"\bint\s+gt_wn_boundary_rev\s*\(\s*const\s+gt_boundary_rev_args\s*\*\s*args\s*,\s*void\s*\*\s*stream\s*\)\s*;", txt)
    assert re.search(r"typedef\s+struct\s+gt_boundary_rev_args\s*\{.*?\}\s*gt_boundary_rev_args\s*;", txt, flags=re.S)


def test_library_exports_the_reverse_boundary_entry(built):
    from glow_tts_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(L, "gt_wn_boundary_rev") and hasattr(L, "gt_boundary_rev_args_size")
    assert "gt_wn_boundary_rev" in _lib.PROTOTYPES


def test_struct_mirror_has_the_c_structs_size_and_fields(built):
    """The ctypes mirror against sizeof() in the library, and its field names in order against the header's declaration."""
    from glow_tts_amd import _lib
    L = _lib.lib()
    assert ctypes.sizeof(_lib.BoundaryRevArgs) == L.gt_boundary_rev_args_size()
    body = re.search(r"typedef\s+struct\s+gt_boundary_rev_args\s*\{(.*?)\}\s*gt_boundary_rev_args\s*;", header_text(), flags=re.S).group(1)
    names = []
    for decl in body.split(";"):
        for part in decl.split(","):
            m = re.search(r"([A-Za-z_][A-Za-z0-9_]*)\s*(?:\[\d+\])?\s*$", part.strip())
            if m:
                names.append(m.group(1))
    assert names == [f[0] for f in _lib.BoundaryRevArgs._fields_]


def test_argument_validation_needs_no_device(built):
    from glow_tts_amd import _lib
    L = _lib.lib()
    assert L.gt_wn_boundary_rev(None, None) == -1                                 # GT_E_INVAL
    a = _lib.BoundaryRevArgs()
    assert L.gt_wn_boundary_rev(ctypes.byref(a), None) == 0                       # R == 0: nothing to do
    a.R = -1
    assert L.gt_wn_boundary_rev(ctypes.byref(a), None) == -1
    a.R, a.H, a.C, a.n_layers = 64, 192, 160, 3                                   # a shape the kernel is not built for
    assert L.gt_wn_boundary_rev(ctypes.byref(a), None) == -1
    a.n_layers = 4                                                                # neither a tail nor a head; no row mask
    assert L.gt_wn_boundary_rev(ctypes.byref(a), None) == -1
    a.h_next, a.rowmask, a.w_start, a.b_start, a.ks_start = 4096, 4096, 4096, 4096, 5
    assert L.gt_wn_boundary_rev(ctypes.byref(a), None) == -1                      # head-only without x_in / z_bct
    a.x_in = 4096 + 4
    assert L.gt_wn_boundary_rev(ctypes.byref(a), None) == -3                      # GT_E_ALIGN
    # gt_wn_stack_fwd: the backward's saves are given for every layer or for none
    s = _lib.WnStackFwdArgs()
    s.R, s.H, s.taps, s.n_layers = 64, 192, 5, 2
    s.x0 = s.rowmask = s.acts = 4096
    s.ldacts = 384
    for i in range(2):
        s.w_in[i] = s.b_in[i] = 4096
    s.w_res[0] = s.b_res[0] = 4096
    s.gate_t[0] = 4096                                                            # one of five: a mix
    assert L.gt_wn_stack_fwd(ctypes.byref(s), None) == -1
