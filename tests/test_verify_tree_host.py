"""CPU-side checks of the draft-tree entry's C-ABI surface (gl3_forward_batch_verify_tree): header, export, ctypes mirror, HipMasterPlan."""
import ctypes
import os
import re

import __graft_entry__ as ge

NAME = "gl3_forward_batch_verify_tree"


def test_header_export_prototype_method_and_null_context(pkg):
    hdr = open(os.path.join(ge.ROOT, "include", "gpullama3_hip.h")).read()
    decl = re.search(r"GL3_API\s+int32_t\s+%s\s*\(([^;]*)\)\s*;" % NAME, hdr)
    assert decl, NAME
    names = [a.split()[-1].lstrip("*") for a in decl.group(1).split(",")]
    assert names == ["ctx", "tokens", "seq_ids", "positions", "parents", "n", "results_out", "path_out", "n_trees_out"]
    if not os.path.exists(os.path.join(ge.PKG_DIR, "libgpullama_hip.so")):
        ge.build()
    ge.load_package()
    from importlib import import_module
    hip = import_module(ge.PKG_NAME + ".hip")
    assert callable(getattr(import_module(ge.PKG_NAME + ".plan").HipMasterPlan, "forward_batch_verify_tree"))
    assert NAME in hip.check_exports()            # header == ctypes table == exported symbols
    restype, argtypes = hip._SIGS[NAME]
    assert restype is ctypes.c_int32 and len(argtypes) == 9 and argtypes[5] is ctypes.c_int32
    getattr(ctypes.CDLL(hip.SO_PATH), NAME)
    assert getattr(hip.lib(), NAME)(None, None, None, None, None, 1, None, None, None) == hip.E_ARG      # a null context, before any device
