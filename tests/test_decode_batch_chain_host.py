"""CPU-side checks of the batched draft chain's C-ABI surface: the header declares gl3_forward_decode_batch_chain and gl3_draft_probs_put_row
and states their contracts, the built library exports both, hip.py binds them with the declared prototypes, HipMasterPlan has the methods,
and csrc/Makefile builds tools/gl3_spec_batch_run from the header and the library.  No device is touched: the calls made pass a null
context, which is refused before any."""
import ctypes
import os
import re

import __graft_entry__ as ge

CHAIN, PUT_ROW = "gl3_forward_decode_batch_chain", "gl3_draft_probs_put_row"


def _hip():
    if not os.path.exists(os.path.join(ge.PKG_DIR, "libgpullama_hip.so")):
        ge.build()
    ge.load_package()
    from importlib import import_module
    return import_module(ge.PKG_NAME + ".hip")


def _header():
    return open(os.path.join(ge.ROOT, "include", "gpullama3_hip.h")).read()


def _declaration(name):
    """(the comment in front of the declaration, the parameter kinds) of a GL3_API entry of the header"""
    h = _header()
    decl = re.search(r"GL3_API\s+int32_t\s+%s\s*\(([^;]*)\)\s*;" % name, h)
    assert decl, "the header does not declare " + name
    params = [re.sub(r"/\*.*?\*/", "", p, flags=re.S).strip() for p in re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")]
    kinds = [" ".join(p.split()[:-1]).replace(" *", "*") + ("*" if p.split()[-1].startswith("*") else "") for p in params]
    doc = h[:decl.start()].rsplit("/*", 1)[1]
    assert doc.rstrip().endswith("*/"), "no comment directly in front of " + name
    return doc, kinds


def test_the_library_exports_both_entries(pkg):
    hip = _hip()
    exported = hip.check_exports()                # header == ctypes table == exported symbols
    for name in (CHAIN, PUT_ROW):
        assert name in exported
        getattr(ctypes.CDLL(hip.SO_PATH), name)
    out = (ctypes.c_int32 * 4)()
    assert hip.lib().gl3_forward_decode_batch_chain(None, None, None, None, 2, 2, None, None, None, None, None, out) == hip.E_ARG
    assert hip.lib().gl3_draft_probs_put_row(None, 0, None, 0) == hip.E_ARG


def test_the_bindings_have_the_declared_prototypes(pkg):
    hip = _hip()
    C = ctypes
    want_kinds = {
        CHAIN: ["gl3_ctx*", "const int32_t*", "const int32_t*", "const int32_t*", "int32_t", "int32_t", "const int32_t*", "const float*",
                "const float*", "gl3_ctx*", "const int32_t*", "int32_t*"],
        PUT_ROW: ["gl3_ctx*", "int32_t", "gl3_ctx*", "int32_t"],
    }
    of = {"int32_t": C.c_int32, "float": C.c_float}
    for name, want in want_kinds.items():
        _, kinds = _declaration(name)
        assert kinds == want, (name, kinds)
        args_want = [of.get(k, C.c_void_p) for k in kinds]          # every pointer is passed as void*, as in the rest of the table
        res, args = hip._SIGS[name]
        assert res is C.c_int32 and args == args_want, name
        fn = getattr(hip.lib(), name)
        assert fn.restype is C.c_int32 and list(fn.argtypes) == args_want, name


def test_the_header_states_the_contracts(pkg):
    doc, _ = _declaration(CHAIN)
    for phrase in ("bit for bit", "gl3_forward_decode_batch_sample", "gl3_draft_probs_put_row(target, slots[i] + j, ctx, i)", "non-increasing",
                   "k_rows[0] == k", "no row is ever compacted", "set to -1", "no top-p", "gl3_get_sample_probs_row", "gl3_get_buffer(3..6)",
                   "gl3_get_attn_rows", "KV contract", "waits once", "4 * k * n bytes", "before anything is uploaded or enqueued",
                   "GL3_E_ARG", "GL3_E_STATE", "GL3_E_UNSUPPORTED", "GL3_CHAIN_MAX", "tp_size > 1"):
        assert phrase in doc, phrase
    doc, _ = _declaration(PUT_ROW)
    for phrase in ("gl3_get_sample_probs_row(draft, row)", "device-to-device copy on the target's stream", "gl3_draft_probs_put", "GL3_E_ARG",
                   "GL3_E_STATE", "GL3_E_UNSUPPORTED", "greedy", "top-p"):
        assert phrase in doc, phrase


def test_the_plan_has_the_methods(pkg):
    _hip()
    from importlib import import_module
    plan = import_module(ge.PKG_NAME + ".plan").HipMasterPlan
    assert callable(getattr(plan, "forward_decode_batch_chain")) and callable(getattr(plan, "draft_probs_put_row"))


def test_the_makefile_builds_the_native_host(pkg):
    mk = open(os.path.join(ge.PKG_DIR, "csrc", "Makefile")).read()
    var = re.search(r"^(\w+)\s*=\s*\.\./\.\./tools/gl3_spec_batch_run\s*$", mk, re.M)
    assert var, "no variable names ../../tools/gl3_spec_batch_run"
    rule = re.search(r"^\$\(%s\):(.*)$" % var.group(1), mk, re.M)
    assert rule, "no rule for the host"
    pre = rule.group(1).split()
    assert "../../tools/gl3_spec_batch_run.cpp" in pre and "../../include/gpullama3_hip.h" in pre and "$(LIB)" in pre, pre
    all_rule = re.search(r"^all:(.*)$", mk, re.M).group(1)
    assert "$(%s)" % var.group(1) in all_rule.split()
    src = open(os.path.join(ge.ROOT, "tools", "gl3_spec_batch_run.cpp")).read()
    for call in (CHAIN + "(", PUT_ROW + "(", "gl3_forward_batch_verify_dist(", '"--no-chain"'):
        assert call in src, call
    assert "tools/gl3_spec_batch_run" in open(os.path.join(ge.ROOT, ".gitignore")).read().split()
