"""CPU (no GPU): the C ABI as Python sees it.  ``_lib.signatures`` reads every declaration of include/clip_event_hip.h,
``_lib.lib`` installs them as ``restype`` / ``argtypes``, a call that disagrees with the header is refused before it
leaves Python, and every call site of the package passes as many arguments as the header declares."""
import ast
import ctypes
import glob
import os
import re

import pytest

from tests.test_micro_batch_cpu import TOWERS, _desc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE_T = ("ce_tower_workspace_bytes", "ce_tower_infer_workspace_bytes", "ce_infonce_workspace_bytes",
          "ce_score_topk_workspace_bytes", "ce_head_small_workspace_floats", "ce_head_small_scalars_offset",
          "ce_preprocess_table_bytes")
VOID = ("ce_profile_enable", "ce_gemm_nt_tune", "ce_gemm_nt_fp8_tune")


def _header() -> str:
    with open(os.path.join(ROOT, "include", "clip_event_hip.h")) as f:
        return f.read()


def _declared():
    from clip_event_amd._lib import signatures
    return signatures(_header())


# ---------------------------------------------------------------------------------------------------------------
# 1. the parse covers the header


def test_signatures_cover_every_declared_symbol():
    names = sorted(set(re.findall(r"\b(ce_[a-z0-9_]+)\s*\(", _header())))      # test_c_abi_exports_every_declared_symbol's set
    sigs = _declared()
    assert sorted(sigs) == names and len(names) >= 100
    void_p, c_int, c_long, c_float = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float
    assert sigs["ce_gemm_tn"] == (c_int, [void_p, c_long, void_p, c_long, c_int, c_int, c_int, void_p, c_long, c_int, void_p])
    assert sigs["ce_cast_t"] == (c_int, [void_p, c_int, void_p, c_int, c_float, c_long, void_p])
    assert sigs["ce_last_error"] == (ctypes.c_char_p, []) and sigs["ce_version"] == (c_int, [])
    assert sigs["ce_gemm_tn_grouped"][1][:5] == [c_int, void_p, void_p, void_p, void_p]     # T* const* and const long*
    assert sigs["ce_profile_collect"] == (c_int, [void_p, c_int])                            # double*


def test_lib_installs_every_signature():
    from clip_event_amd._lib import lib
    cl = lib()
    for name, (restype, argtypes) in _declared().items():
        fn = getattr(cl, name)
        assert fn.argtypes is not None and list(fn.argtypes) == argtypes, name
        assert fn.restype is restype, name
    for name in SIZE_T:
        assert getattr(cl, name).restype is ctypes.c_size_t, name
    assert cl.ce_cu_hog_clock_mhz.restype is ctypes.c_double
    assert cl.ce_last_error.restype is ctypes.c_char_p and cl.ce_profile_class_name.restype is ctypes.c_char_p
    for name in VOID:
        assert getattr(cl, name).restype is None, name
    assert {n for n, (r, _) in _declared().items() if r is None} == set(VOID)


@pytest.mark.parametrize("decl, named", [("int ce_new_thing(const float* x, short x, void* stream);", "ce_new_thing"),
                                         ("int ce_other(unsigned int flags);", "ce_other"),
                                         ("float* ce_returns_pointer(int n);", "ce_returns_pointer"),
                                         ("ce_nt_plan ce_by_value(int n);", "ce_by_value")])
def test_signatures_refuse_a_type_outside_the_table(decl, named):
    from clip_event_amd._lib import signatures
    with pytest.raises(TypeError, match=named):
        signatures("int ce_fine(int a, long b);\n/* a comment (with parentheses); */\n" + decl)


def test_missing_header_is_an_error_at_load(monkeypatch, tmp_path):
    from clip_event_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "HEADER", str(tmp_path / "clip_event_hip.h"))
    with pytest.raises(FileNotFoundError, match="clip_event_hip.h"):
        _lib.lib()
    assert _lib._lib is None


# ---------------------------------------------------------------------------------------------------------------
# 2. a call that disagrees with the header does not leave Python


def test_plan_call_refuses_a_wrong_width_and_a_missing_argument():
    from clip_event_amd._lib import NTPlan, lib
    cl = lib()
    plan = NTPlan()
    good = (4000, 768, 768, 0, 0, 768, 768, 768, 0, 0, 0, ctypes.byref(plan))
    with pytest.raises(ctypes.ArgumentError):
        cl.ce_gemm_nt_plan(ctypes.c_long(4000), *good[1:])
    with pytest.raises(TypeError):
        cl.ce_gemm_nt_plan(*good[:-1])
    assert plan.block == 0 and plan.workgroups == 0
    assert cl.ce_gemm_nt_plan(*good) == 0
    assert plan.taken == 1 and plan.block > 0 and plan.workgroups > 0 and plan.tiles_m * plan.tiles_n > 0


WG_SETS, LNP_RING = 9, 8        # csrc/tower.cpp


def _training_workspace_bytes(cl, layers, width, heads, tokens, stream16, fp8, batch):
    """``carve`` of csrc/tower.cpp in Python integers: every buffer starts on a 256-byte boundary."""
    off = 0

    def take(nbytes):
        nonlocal off
        off = (off + 255) // 256 * 256 + nbytes

    M, w, esz = batch * tokens, width, 2 if stream16 else 4
    for layer in range(layers):
        take(M * w * esz)                                           # x_mid
        if layer + 1 < layers:
            take(M * w * esz)                                       # x_out
        for cols in (1, 3, 1, 1, 4, 4):                             # h1, qkv, o, h2, a, g
            take(M * cols * w * 2)
        for _ in range(4):                                          # LayerNorm statistics
            take(M * 4)
        take(batch * heads * tokens * 4)                            # lse
    for _ in range(WG_SETS):
        for cols in (1, 1, 4, 3):                                   # dxb, dxb2, da, dqkv
            take(M * cols * w * 2)
    take(M * w * 2), take(M * w * 2)                                # dh, d_o
    if fp8:
        take(M * 4 * w), take(M * 4)
    for _ in range(3):                                              # xs_in, xs_mid, dxs_mid
        take(batch * w * 4)
    take(batch * 4), take(batch * 4)
    for cols in (1, 1, 4, 4, 1, 1, 4, 1, 1):                        # os, h2s, as, gs, dxbs, dxb2s, das, dhs, dos
        take(batch * cols * w * 2)
    lnp_bytes = cl.ce_layernorm_bwd_blocks(M, w) * 3 * w * 4
    for slot in range(min(LNP_RING, layers)):
        take(lnp_bytes), take(lnp_bytes)
    return (off + 255) // 256 * 256


def test_workspace_size_above_4_gib_is_not_truncated():
    from clip_event_amd._lib import lib
    cl = lib()
    width, heads, tokens, causal = TOWERS["vit_l14_336"]
    for layers, stream16, fp8, batch in ((24, 0, 0, 16), (24, 1, 3, 16), (2, 0, 0, 4)):
        expect = _training_workspace_bytes(cl, layers, width, heads, tokens, stream16, fp8, batch)
        got = cl.ce_tower_workspace_bytes(ctypes.byref(_desc(layers, width, heads, tokens, causal, stream16, fp8)), batch)
        print(f"layers {layers} stream16 {stream16} fp8 {fp8} batch {batch}: {got} bytes, layout arithmetic {expect}")
        assert got == expect
        assert (expect > 1 << 32) == (layers == 24)


# ---------------------------------------------------------------------------------------------------------------
# 3. every call site of the package agrees with the header

WRAPPERS = ("c_int", "c_long", "c_float")
# (file, function) -> number of positional arguments a ``*splat`` contributes, for the splats the walk cannot size itself
EXPLICIT_SPLATS = {}


def _literal_length(node):
    if isinstance(node, (ast.Tuple, ast.List)) and not any(isinstance(e, ast.Starred) for e in node.elts):
        return len(node.elts)
    return None


def _splat_length(value, module, scope):
    """Length of ``*value`` where it is static: a name the enclosing function assigns once, to a list / tuple display, or a
    call of a module-level function whose only ``return`` is a tuple display."""
    if isinstance(value, ast.Name):
        assigned = [n.value for n in ast.walk(scope) if isinstance(n, ast.Assign)
                    and any(isinstance(t, ast.Name) and t.id == value.id for t in n.targets)]
        return _literal_length(assigned[0]) if len(assigned) == 1 else None
    if isinstance(value, ast.Call) and isinstance(value.func, ast.Name):
        defs = [n for n in module.body if isinstance(n, ast.FunctionDef) and n.name == value.func.id]
        returns = [n.value for d in defs for n in ast.walk(d) if isinstance(n, ast.Return)]
        return _literal_length(returns[0]) if len(returns) == 1 else None
    return None


def _abi_calls(path, declared):
    """(function name, line, positional argument count or None, wrapped arguments) of every ``<expr>.ce_*(...)`` call."""
    with open(path) as f:
        module = ast.parse(f.read(), path)
    scopes = [n for n in ast.walk(module) if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef))]
    for call in (n for n in ast.walk(module) if isinstance(n, ast.Call)):
        if not (isinstance(call.func, ast.Attribute) and call.func.attr in declared):
            continue
        inside = [s for s in scopes if any(n is call for n in ast.walk(s))]
        scope = min(inside, key=lambda s: s.end_lineno - s.lineno) if inside else module
        count = 0
        for arg in call.args:
            if isinstance(arg, ast.Starred):
                n = _splat_length(arg.value, module, scope)
                if n is None:
                    n = EXPLICIT_SPLATS.get((os.path.basename(path), call.func.attr))
                count = None if (n is None or count is None) else count + n
            elif count is not None:
                count += 1
        wrapped = [ast.unparse(a) for a in ast.walk(call) if isinstance(a, ast.Call) and a is not call
                   and (getattr(a.func, "id", None) in WRAPPERS or getattr(a.func, "attr", None) in WRAPPERS)]
        yield call.func.attr, call.lineno, count, wrapped, bool(call.keywords)


def test_every_package_call_site_passes_what_the_header_declares():
    declared = _declared()
    files = sorted(glob.glob(os.path.join(ROOT, "clip_event_amd", "*.py")))
    seen, problems = set(), []
    for path in files:
        for name, line, count, wrapped, keywords in _abi_calls(path, declared):
            where = f"{os.path.basename(path)}:{line} {name}"
            seen.add(name)
            if count is None:
                problems.append(f"{where}: a *splat of unknown length (size it in EXPLICIT_SPLATS)")
            elif count != len(declared[name][1]):
                problems.append(f"{where}: {count} arguments, the header declares {len(declared[name][1])}")
            if wrapped:
                problems.append(f"{where}: hand-wrapped arguments {wrapped}")
            if keywords:
                problems.append(f"{where}: keyword arguments")
    assert not problems, "\n".join(problems)
    # the walk saw the call sites it is there for: the step's hot path and the splatted GEMM tails
    assert {"ce_gemm_nt", "ce_gemm_nt_fp8", "ce_gemm_nt_mx8", "ce_gemm_tn", "ce_layernorm_fwd_t", "ce_layernorm_bwd_t",
            "ce_tower_forward", "ce_tower_backward_range", "ce_l2norm_fwd", "ce_infonce_fwd", "ce_gemm_nt_plan"} <= seen
    assert len(seen) >= 60
    for path in files:                    # return types are set in one place
        with open(path) as f:
            text = f.read()
        assert ".restype" not in text or os.path.basename(path) == "_lib.py", path
    # each of these argument lists is written once in the package
    for name in ("ce_gemm_nt", "ce_gemm_tn", "ce_layernorm_fwd_t", "ce_layernorm_bwd_t", "ce_l2norm_fwd", "ce_l2norm_bwd"):
        sites = [(os.path.basename(p), line) for p in files for n, line, *_ in _abi_calls(p, declared) if n == name]
        assert len(sites) == 1, (name, sites)
