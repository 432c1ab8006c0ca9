"""CPU-side checks of the draft chain's C-ABI surface: the header declares gl3_forward_decode_chain and GL3_CHAIN_MAX and states the contract,
the built library exports the symbol, hip.py binds it with the declared prototype and mirrors the constant, HipMasterPlan has the method, and
the native host knows --chain.  No device is touched: the one call made passes a null context, which is refused before any."""
import ctypes
import os
import re

import __graft_entry__ as ge

NAME = "gl3_forward_decode_chain"


def _hip():
    if not os.path.exists(os.path.join(ge.PKG_DIR, "libgpullama_hip.so")):
        ge.build()
    ge.load_package()
    from importlib import import_module
    return import_module(ge.PKG_NAME + ".hip")


def _header():
    return open(os.path.join(ge.ROOT, "include", "gpullama3_hip.h")).read()


def test_the_library_exports_the_entry(pkg):
    hip = _hip()
    assert NAME in hip.check_exports()            # header == ctypes table == exported symbols
    getattr(ctypes.CDLL(hip.SO_PATH), NAME)
    out = (ctypes.c_int32 * 2)()
    assert hip.lib().gl3_forward_decode_chain(None, 0, 0, 2, 0.0, None, None, 0, out) == hip.E_ARG      # a null context, before any device


def test_the_binding_has_the_declared_prototype(pkg):
    hip = _hip()
    C = ctypes
    decl = re.search(r"GL3_API\s+int32_t\s+%s\s*\(([^;]*)\)\s*;" % NAME, _header())
    assert decl, "the header does not declare " + NAME
    params = [re.sub(r"/\*.*?\*/", "", p).strip() for p in decl.group(1).split(",")]
    kinds = [" ".join(p.split()[:-1]).replace(" *", "*") + ("*" if p.split()[-1].startswith("*") else "") for p in params]
    assert kinds == ["gl3_ctx*", "int32_t", "int32_t", "int32_t", "float", "const float*", "gl3_ctx*", "int32_t", "int32_t*"], kinds
    of = {"int32_t": C.c_int32, "float": C.c_float}
    want = [of.get(k, C.c_void_p) for k in kinds]          # every pointer is passed as void*, as in the rest of the table
    res, args = hip._SIGS[NAME]
    assert res is C.c_int32 and args == want
    fn = getattr(hip.lib(), NAME)
    assert fn.restype is C.c_int32 and list(fn.argtypes) == want


def test_chain_max_is_mirrored(pkg):
    hip = _hip()
    m = re.search(r"^#define\s+GL3_CHAIN_MAX\s+(\d+)\s*$", _header(), re.M)
    assert m and int(m.group(1)) == hip.CHAIN_MAX == 64


def test_the_header_states_the_contract(pkg):
    doc = _header().split("#define GL3_CHAIN_MAX")[0].rsplit("/*", 1)[1]
    for phrase in ("bit for bit", "gl3_forward_decode_sample", "gl3_draft_probs_put", "KV contract", "GL3_E_ARG", "GL3_E_STATE", "GL3_E_UNSUPPORTED", "ONE-rank"):
        assert phrase in doc, phrase


def test_the_plan_and_the_native_host_have_it(pkg):
    _hip()
    from importlib import import_module
    assert callable(getattr(import_module(ge.PKG_NAME + ".plan").HipMasterPlan, "forward_decode_chain"))
    src = open(os.path.join(ge.ROOT, "tools", "gl3_spec_draft_run.cpp")).read()
    assert '"--chain"' in src and NAME + "(" in src
