"""CPU tests of the long-text front end of synthesis: gt_synth_lengths_long, gt_synth_prior_long and
gt_synth_prior_long_call are declared, exported and bound as the header declares them, refuse what their short siblings refuse — with
the token limit at GT_SYNTH_LONG_MAX_TX = 4096 — and gt_attn_fwd takes P == NULL at the shapes of the key-tiled kernel only.  Every
call below returns before a launch: no device is needed."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVAL, UNSUPPORTED, ALIGN = -1, -2, -3
P = 4096                                                                          # a non-NULL, 16-byte aligned "pointer" that is never read
NEW = ("gt_synth_lengths_long", "gt_synth_prior_long", "gt_synth_prior_long_call")


def header_text():
    txt = open(os.path.join(ROOT, "include", "glowtts_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def c_class(decl):
    from glow_tts_amd import _lib
    if "*" in decl:
        return _lib.Pointer
    words = [w for w in decl.replace("const", " ").split() if w in ("int", "int32_t")]
    assert len(words) == 1, f"unclassified C type in {decl!r}"
    return ctypes.c_int


def test_header_declares_the_entries_and_the_limit():
    txt = header_text()
    assert int(re.search(r"#define\s+GT_SYNTH_LONG_MAX_TX\s+(\d+)", txt).group(1)) == 4096
    assert int(re.search(r"#define\s+GT_ATTN_LONG_MAX_T\s+(\d+)", txt).group(1)) == 4096
    assert re.search(r"\bint\s+gt_synth_lengths_long\s*\(\s*const\s+float\s*\*\s*dur\s*,\s*const\s+int32_t\s*\*\s*x_len\s*,\s*int32_t\s*\*\s*cum\s*,"
                     r"\s*int32_t\s*\*\s*y_len\s*,\s*float\s*\*\s*logw\s*,\s*int\s+B\s*,\s*int\s+Tx\s*,\s*void\s*\*\s*stream\s*\)\s*;", txt)
    assert re.search(r"\bint\s+gt_synth_prior_long\s*\(\s*const\s+gt_synth_prior_args\s*\*\s*args\s*,\s*void\s*\*\s*stream\s*\)\s*;", txt)
    assert re.search(r"\bint\s+gt_synth_prior_long_call\s*\(\s*const\s+gt_synth_prior_args\s*\*\s*args\s*,\s*const\s+gt_synth_call\s*\*\s*call\s*,"
                     r"\s*void\s*\*\s*stream\s*\)\s*;", txt)


def test_library_exports_and_binding_match_the_header(built):
    from glow_tts_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    decls = {n: (r, p) for r, n, p in re.findall(r"([\w \t\*]+?)\b(gt_\w+)\s*\(([^;{}()]*)\)\s*;", header_text())}
    for name in NEW:
        assert hasattr(L, name) and name in _lib.PROTOTYPES and name in decls, name
        res, args = _lib.PROTOTYPES[name]
        assert res is _lib.STATUS and c_class(decls[name][0]) is ctypes.c_int
        plist = decls[name][1].split(",")
        assert len(plist) == len(args), name
        for prm, cls in zip(plist, args):
            assert c_class(prm) is cls, (name, prm)
        assert callable(getattr(_lib.call, name))                                 # bound on the checked path
    assert _lib.SYNTH_LONG_MAX_TX == 4096 and _lib.SYNTH_MAX_TX == 512
    assert ctypes.sizeof(_lib.SynthPriorArgs) == _lib.lib().gt_synth_prior_args_size()          # the struct keeps its layout


def test_lengths_long_refusals_need_no_device(built):
    from glow_tts_amd import _lib
    f = _lib.lib().gt_synth_lengths_long
    assert f(P, P, P, P, None, 2, 4097, None) == UNSUPPORTED
    assert f(P, P, P, P, P, 2, 100000, None) == UNSUPPORTED
    assert f(P, P, P, P, None, 2, 0, None) == INVAL
    assert f(P, P, P, P, None, -1, 600, None) == INVAL
    assert f(None, None, None, None, None, 0, 600, None) == 0                     # B == 0
    for i in range(4):                                                            # dur, x_len, cum, y_len are required; logw is not
        a = [P] * 4
        a[i] = None
        assert f(*a, None, 2, 600, None) == INVAL, i
        assert f(*a, None, 2, 4097, None) == INVAL, i                             # as the short entry: NULL is named before the limit


def prior_args(_lib, Tx=600):
    a = _lib.SynthPriorArgs()
    a.R, a.B, a.C, a.Tx, a.Ty, a.Tp = 128, 3, 80, Tx, 64, 36 + 127
    a.x_m = a.cum = a.x_len = a.y_len = a.rows = a.row0 = P
    return a


def both(L, a, call=P):
    """the status of gt_synth_prior_long and gt_synth_prior_long_call on the same arguments: they must agree"""
    r1, r2 = L.gt_synth_prior_long(ctypes.byref(a), None), L.gt_synth_prior_long_call(ctypes.byref(a), call, None)
    assert r1 == r2, (r1, r2)
    return r1


def test_prior_long_refusals_need_no_device(built):
    from glow_tts_amd import _lib
    L = _lib.lib()
    assert L.gt_synth_prior_long(None, None) == INVAL and L.gt_synth_prior_long_call(None, P, None) == INVAL
    assert both(L, _lib.SynthPriorArgs(), call=None) == 0                         # R == 0 (and B == 0): nothing to do
    a = prior_args(_lib)
    a.B = 0
    assert both(L, a, call=None) == 0
    a = prior_args(_lib)
    a.R = 0
    assert both(L, a, call=None) == 0
    assert both(L, prior_args(_lib, 4097)) == UNSUPPORTED
    assert both(L, prior_args(_lib, 0)) == INVAL
    a = prior_args(_lib)
    a.C = 81
    assert both(L, a) == UNSUPPORTED
    for field in ("x_m", "cum", "x_len", "y_len", "rows"):                        # every required pointer
        a = prior_args(_lib)
        setattr(a, field, None)
        assert both(L, a) == INVAL, field
    a = prior_args(_lib)
    a.x_m = P + 4
    assert both(L, a) == ALIGN
    a = prior_args(_lib)
    a.rows = P + 8
    assert both(L, a) == ALIGN
    a = prior_args(_lib)
    a.row0 = None                                                                 # uniform rows: R must be B * Tp
    assert both(L, a) == INVAL
    a = prior_args(_lib)
    assert L.gt_synth_prior_long_call(ctypes.byref(a), None, None) == INVAL       # no call block
    assert L.gt_synth_prior_long_call(ctypes.byref(a), P + 2, None) == ALIGN
    # the short entries keep their limit
    assert L.gt_synth_prior(ctypes.byref(prior_args(_lib, 513)), None) == UNSUPPORTED
    assert L.gt_synth_prior_call(ctypes.byref(prior_args(_lib, 513)), P, None) == UNSUPPORTED
    assert L.gt_synth_lengths(P, P, P, P, None, 2, 513, None) == UNSUPPORTED


def attn_fwd(L, T, D=96, win=4, P_=None, B=1, H=2):
    return L.gt_attn_fwd(P, P, P, 3 * H * D, P, P, P, P, H * D, P_, B, T, T + 2, None, H, D, win, 0.0, 0, None, None)


def test_attn_fwd_takes_a_null_p_at_long_shapes_only(built):
    from glow_tts_amd import _lib
    L = _lib.lib()
    assert attn_fwd(L, 505) == INVAL                                              # the last T of the generic kernels
    assert attn_fwd(L, 600, D=64) == INVAL                                        # not the key-tiled kernel's head shape
    assert attn_fwd(L, 384) == INVAL                                              # the T <= 384 MFMA kernels
    assert attn_fwd(L, 600, win=3) == INVAL
    assert attn_fwd(L, 4097) == UNSUPPORTED
    assert attn_fwd(L, 4097, P_=P) == UNSUPPORTED


def test_host_mirror_of_the_long_shape_predicate(built):
    from glow_tts_amd import _lib, encoder_impl
    L = _lib.lib()
    for T in (1, 384, 385, 505, 506, 512, 4096, 4097):
        for D_ in (96, 64):
            for win in (4, 3):
                assert bool(L.gt_attn_long_shape(T, D_, win)) == encoder_impl.attn_long_shape(T, D_, win), (T, D_, win)


def test_entries_are_picked_by_token_count():
    """to 512 tokens a call launches the entries it always launched"""
    from glow_tts_amd import synthesis
    assert synthesis._by_tokens("gt_synth_lengths", 512) == "gt_synth_lengths"
    assert synthesis._by_tokens("gt_synth_lengths", 513) == "gt_synth_lengths_long"
    assert synthesis._by_tokens("gt_synth_prior", 19) == "gt_synth_prior" and synthesis._by_tokens("gt_synth_prior", 4096) == "gt_synth_prior_long"
    assert synthesis._by_tokens("gt_synth_prior_call", 512) == "gt_synth_prior_call"
    assert synthesis._by_tokens("gt_synth_prior_call", 520) == "gt_synth_prior_long_call"
