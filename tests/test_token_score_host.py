"""CPU-side checks of the token-score C-ABI (gl3_forward_batch_score, gl3_score_rows): the header declares both entries and the 16-byte
gl3_token_score record, the library exports them, the ctypes mirror and HipMasterPlan know them, each refuses a null context before
anything touches a device, and the Makefile builds the native perplexity host."""
import ctypes
import os
import re

import numpy as np

import __graft_entry__ as ge

NEW = ["gl3_forward_batch_score", "gl3_score_rows"]


def _hip():
    if not os.path.exists(os.path.join(ge.PKG_DIR, "libgpullama_hip.so")):
        ge.build()
    ge.load_package()
    from importlib import import_module
    return import_module(ge.PKG_NAME + ".hip")


def test_the_header_declares_the_entries_and_the_record(pkg):
    hdr = open(os.path.join(ge.ROOT, "include", "gpullama3_hip.h")).read()
    assert re.search(r"typedef\s+struct\s*\{\s*float\s+prob\s*,\s*logit\s*,\s*max\s*,\s*sum\s*;\s*\}\s*gl3_token_score\s*;", hdr)
    for name in NEW:
        assert re.search(r"GL3_API\s+int32_t\s+%s\s*\(" % name, hdr), name
    from importlib import import_module
    _hip()
    plan_mod = import_module(ge.PKG_NAME + ".plan")
    assert plan_mod.SCORE_DTYPE.itemsize == 16 and plan_mod.SCORE_DTYPE.names == ("prob", "logit", "max", "sum")
    assert all(plan_mod.SCORE_DTYPE[f] == np.float32 for f in plan_mod.SCORE_DTYPE.names)


def test_the_library_exports_the_token_scores(pkg):
    hip = _hip()
    names = hip.check_exports()                   # header == ctypes table == exported symbols
    raw = ctypes.CDLL(hip.SO_PATH)
    for name in NEW:
        assert name in names and name in hip._SIGS
        getattr(raw, name)


def test_a_null_context_is_an_argument_error(pkg):
    hip = _hip()
    L = hip.lib()
    assert L.gl3_forward_batch_score(None, None, None, None, None, 1, None, None, None, None) == hip.E_ARG
    assert L.gl3_score_rows(None, None, 1, None, None, None) == hip.E_ARG


def test_the_plan_mirrors_both_entries(pkg):
    _hip()
    from importlib import import_module
    plan_mod = import_module(ge.PKG_NAME + ".plan")
    for name in ("forward_batch_score", "score_rows"):
        assert callable(getattr(plan_mod.HipMasterPlan, name))


def test_the_makefile_builds_the_perplexity_host(pkg):
    mk = open(os.path.join(ge.PKG_DIR, "csrc", "Makefile")).read()
    assert re.search(r"^PERPLEXITY\s*=\s*\.\./\.\./tools/gl3_perplexity\s*$", mk, re.M)
    assert re.search(r"^all:.*\$\(PERPLEXITY\)", mk, re.M)
    assert re.search(r"^\$\(PERPLEXITY\):\s*\.\./\.\./tools/gl3_perplexity\.cpp\b", mk, re.M)
    assert os.path.exists(os.path.join(ge.ROOT, "tools", "gl3_perplexity.cpp"))
