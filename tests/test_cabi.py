"""CPU tests: the C-ABI shared library loads and exports every symbol include/*.h declares
(no compute calls without a GPU), and the Python binding table matches the header."""
import ctypes
import glob
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    names = []
    for h in glob.glob(os.path.join(ROOT, "include", "*.h")):
        txt = open(h).read()
        txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
        names += re.findall(r"\b(gt_[a-z0-9_]+)\s*\(", txt)
    return sorted(set(names))


def test_header_declares_something():
    syms = declared_symbols()
    assert "gt_mas_f32" in syms and "gt_version" in syms


def test_library_exports_every_declared_symbol(built):
    from glow_tts_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    for s in declared_symbols():
        assert hasattr(L, s), f"{s} declared in include/ but not exported"


def test_binding_table_matches_header(built):
    from glow_tts_amd import _lib
    assert sorted(_lib.PROTOTYPES) == declared_symbols()
    L = _lib.lib()
    assert b"gfx950" in L.gt_version()


def test_host_helpers_no_gpu(built):
    from glow_tts_amd import _lib
    L = _lib.lib()
    # LDS sizing helper is pure host code
    assert L.gt_mas_lds_bytes(150, 800) < 160 * 1024
    assert L.gt_mas_lds_bytes(375, 870) < 160 * 1024
    assert L.gt_mas_lds_bytes(0, 10) == 0
    assert L.gt_mas_workspace_bytes(32, 150, 800) >= 32 * 151 * 4
    # argument validation happens before any launch
    assert L.gt_mas_f32(None, None, None, None, None, 0, None, None, 2, 8, 8, 64, 8, None, 0, None, None) == -1
    assert L.gt_mas_f32(None, None, None, None, None, 0, None, None, 0, 8, 8, 64, 8, None, 0, None, None) == 0
    assert L.gt_mas_f32(None, None, None, None, None, 0, None, None, -1, 8, 8, 64, 8, None, 0, None, None) == -1


def test_ops_fail_loudly_without_gpu(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from glow_tts_amd import monotonic_align
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        monotonic_align.maximum_path(torch.zeros(1, 2, 3), torch.ones(1, 2, 3))


def test_wgrad_planner_slabs_cover_the_rows_and_fill_short_launches():
    """glow_tts_amd.wgrad.WgradQueue._plan (host logic, no GPU): every job's row slabs are 64-row multiples that cover its rows exactly
    once, the partial-sum workspace has room for all of them, and a launch with few short jobs (the duration predictor's two convs)
    is cut into enough tiles to cover the chip — the form that once left a dozen workgroups walking all the rows; the slab counts of
    the bench's two big launches are the measured optima (round 3: 1 slab for the decoder's 432 k = 5 tiles, 2 for its 180 k = 1 tiles)."""
    import types

    import torch
    from glow_tts_amd import wgrad

    def conv(cout, cin, taps):
        pc = types.SimpleNamespace(taps=taps, Cin=cin, Cout=cout, inv_norm=None)
        return types.SimpleNamespace(pc=pc, weight_norm=False, weight=torch.zeros(cout, cin, taps), bias=torch.zeros(cout))

    def plan(shapes, R):
        q = wgrad.WgradQueue(torch.device("cpu"))
        for cout, cin, taps in shapes:
            c = conv(cout, cin, taps)
            q.add(c, R, [(torch.zeros(R, cin, dtype=torch.bfloat16), torch.zeros(R, cout, dtype=torch.bfloat16), 0, cout)])
        return q._plan()

    assert wgrad.choose_slabs(432, 8896, 48 * 5 * 384 * 192 * 4) == 1 and wgrad.choose_slabs(180, 8896, 14_600_000) == 2
    assert wgrad.choose_slabs(14, 3584, 2_000_000) >= 8
    for shapes, R in (([(256, 192, 3), (256, 256, 3)], 3584), ([(256, 192, 3), (256, 256, 3)], 8704),
                      ([(384, 192, 5)] * 48, 9216), ([(192, 192, 5)] * 3, 4096), ([(8, 256, 1)], 4096)):
        jobs, tiles, wnbs, rows, max_n, nbytes = plan(shapes, R)
        assert len(jobs) == len(shapes) and rows == sum(s[0] for s in shapes)
        end = 0
        for (xp, dyp, part_off, pb_off, ldx, ldy, r, cin, cout, co_begin, co_count, slab_rows), w in zip(jobs, wnbs):
            S = w[8]
            taps = w[11]
            assert r == R and slab_rows % 64 == 0 and (S - 1) * slab_rows < R <= S * slab_rows
            assert part_off >= end and pb_off >= part_off + S * taps * cout * cin * 4          # partials, then the bias partials
            end = pb_off + S * cout * 4
        assert nbytes >= end
        for taps in (5, 3, 1):
            n_tiles = sum(nco * nci * S for _, _, nco, nci, S in tiles[taps])
            base = sum(nco * nci for _, _, nco, nci, S in tiles[taps])
            if base:
                # a launch is either one full round of the chip's 512 workgroup slots (or more, uncut), or cut until its slabs are short
                S = max(S for _, _, _, _, S in tiles[taps])
                assert n_tiles >= 0.6 * wgrad.SLOTS or S >= min(8, R // 128) or base >= wgrad.SLOTS // 2, (shapes[0], R, n_tiles, S)


# ---- the binding table and the structure mirrors against include/glowtts_hip.h ----------------------------------------------------
def header_text():
    txt = open(os.path.join(ROOT, "include", "glowtts_hip.h")).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))


def c_class(decl):
    """a parameter or return type of the header as the class the binding table must hold: anything with * is a pointer"""
    from glow_tts_amd import _lib
    if "*" in decl:
        return _lib.Pointer
    scalars = {"int": ctypes.c_int, "int32_t": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "float": ctypes.c_float,
               "uint32_t": ctypes.c_uint32}
    words = [w for w in decl.replace("const", " ").split() if w in scalars]
    assert len(words) == 1, f"unclassified C type in {decl!r}"
    return scalars[words[0]]


def test_prototypes_match_the_header_declarations():
    """every `ret gt_name(params);` of the header against PROTOTYPES[name]: parameter count, order and class, and the return type
    (a status entry is an int in C; which int-returning entries are statuses is the table's own statement)"""
    from glow_tts_amd import _lib
    decls = re.findall(r"([\w \t\*]+?)\b(gt_\w+)\s*\(([^;{}()]*)\)\s*;", header_text())
    assert sorted(n for _, n, _ in decls) == sorted(_lib.PROTOTYPES) and len(decls) == len(_lib.PROTOTYPES)
    for ret, name, params in decls:
        res, args = _lib.PROTOTYPES[name]
        ret = ret.replace("GT_API", " ").replace("extern", " ")
        want_res = ctypes.c_char_p if ("char" in ret and "*" in ret) else c_class(ret)
        assert (ctypes.c_int if res is _lib.STATUS else res) is want_res, f"{name}: return type {ret.strip()!r} vs {res}"
        plist = [] if params.strip() in ("", "void") else params.split(",")
        assert len(plist) == len(args), f"{name}: {len(plist)} parameters in the header, {len(args)} in PROTOTYPES"
        for i, (prm, cls) in enumerate(zip(plist, args)):
            assert c_class(prm) is cls, f"{name}: parameter {i} is {' '.join(prm.split())!r} in the header, {cls.__name__} in PROTOTYPES"


def test_struct_mirrors_match_the_header_layout(tmp_path):
    """sizeof and every offsetof of every mirror (the ctypes structures of _lib, the numpy record types of wgrad), as a C compiler
    lays the header's structs out, against ctypes / numpy; a field the header lacks does not compile"""
    from glow_tts_amd import _lib, wgrad
    mirrors = [(cname, ctypes.sizeof(cls), [(f[0], getattr(cls, f[0]).offset) for f in cls._fields_]) for cls, cname in _lib.C_STRUCTS.items()]
    mirrors += [(cname, dt.itemsize, [(f, dt.fields[f][1]) for f in dt.names]) for cname, dt in wgrad.C_STRUCTS.items()]
    assert len(_lib.C_STRUCTS) == sum(isinstance(v, type) and issubclass(v, ctypes.Structure) for v in vars(_lib).values())
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "glowtts_hip.h"', 'int main(void) {']
    for cname, _, fields in mirrors:
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'  printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in fields]
    lines += ['  return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([os.environ.get("CC", "gcc"), "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    want = {}
    for cname, size, fields in mirrors:
        want[cname] = str(size)
        want.update({f"{cname}.{f}": str(off) for f, off in fields})
    assert got == want, {k: (got.get(k), want[k]) for k in want if got.get(k) != want[k]}


def test_checked_call_path(built):
    """_lib.call on entries that return before any launch: statuses raise GtError, values come back, tensors / structures / byref /
    None all convert, and record_calls sees the entry"""
    import torch
    from glow_tts_amd import _lib
    call, L = _lib.call, _lib.lib()
    a = _lib.BoundaryRevArgs()
    assert a.R == 0 and call.gt_wn_boundary_rev(a, None) is None
    a.R = -1
    with pytest.raises(_lib.GtError) as ei:
        call.gt_wn_boundary_rev(a, None)
    assert (ei.value.entry, ei.value.code, str(ei.value)) == ("gt_wn_boundary_rev", -1, "gt_wn_boundary_rev failed: GT_E_INVAL")
    assert isinstance(ei.value, RuntimeError)
    assert L.gt_wn_boundary_rev(a, None) == L.gt_wn_boundary_rev(ctypes.byref(a), None) == -1
    a.R = 0
    assert L.gt_wn_boundary_rev(a, None) == L.gt_wn_boundary_rev(ctypes.byref(a), None) == 0
    assert call.gt_mas_lds_bytes(150, 800) == L.gt_mas_lds_bytes(150, 800) > 0
    # a tensor is passed as its address: the slab count lands in the tensor's own memory
    R, Cin, Cout, taps = 9216, 192, 384, 5
    S, t = ctypes.c_int(0), torch.zeros(1, dtype=torch.int32)
    nbytes = L.gt_conv_wgrad_workspace_bytes(R, Cin, Cout, taps, ctypes.byref(S))
    assert call.gt_conv_wgrad_workspace_bytes(R, Cin, Cout, taps, t) == nbytes > 0
    assert S.value >= 1 and int(t[0]) == S.value
    with _lib.record_calls() as names:
        call.gt_mas_lds_bytes(150, 800)
        call.gt_wn_boundary_rev(a, None)
    assert names == ["gt_mas_lds_bytes", "gt_wn_boundary_rev"]


def test_product_code_uses_the_checked_path():
    """outside _lib.py the package calls the library through _lib.call only: no raw lib() / check / ptr"""
    for path in sorted(glob.glob(os.path.join(ROOT, "glow-tts_amd", "*.py"))):
        if os.path.basename(path) == "_lib.py":
            continue
        src = open(path).read()
        assert not re.search(r"_lib\.(lib|check|ptr)\b", src), path
        for m in re.finditer(r"from\s+\.?_lib\s+import\s+([^\n]+)", src):
            assert not {"lib", "check", "ptr"} & {w.strip().split(" as ")[0] for w in m.group(1).strip("() ").split(",")}, path


@pytest.mark.gpu
def test_checked_path_hands_the_kernel_the_device_address(built):
    """gt_randn_rows (R = 3, ncol = 5: the odd column count takes the tail store) through the raw surface with _lib.ptr and through
    _lib.call with the tensor itself: bit-equal buffers"""
    import torch
    from glow_tts_amd import _lib
    dev = torch.device("cuda:0")
    R, ncol, seed, stream_id, scale = 3, 5, 1234, 2, 0.75
    raw = torch.zeros(R, ncol, dtype=torch.float32, device=dev)
    via = torch.zeros(R, ncol, dtype=torch.float32, device=dev)
    assert _lib.lib().gt_randn_rows(_lib.ptr(raw), R, ncol, seed, stream_id, scale, _lib.current_stream(dev)) == 0
    _lib.call.gt_randn_rows(via, R, ncol, seed, stream_id, scale, _lib.current_stream(dev))
    torch.cuda.synchronize()
    assert raw.abs().sum().item() > 0 and torch.equal(raw.view(torch.int32), via.view(torch.int32))
