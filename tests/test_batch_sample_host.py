"""CPU-side checks of the batched sampler's C-ABI (gl3_forward_decode_batch_sample, gl3_get_sample_probs_row, gl3_sample_rows):
the library exports the three entry points the header declares, the ctypes mirror knows them, and each refuses a null context
before anything touches a device."""
import ctypes
import os

import __graft_entry__ as ge

NEW = ["gl3_forward_decode_batch_sample", "gl3_get_sample_probs_row", "gl3_sample_rows"]


def _hip():
    if not os.path.exists(os.path.join(ge.PKG_DIR, "libgpullama_hip.so")):
        ge.build()
    ge.load_package()
    from importlib import import_module
    return import_module(ge.PKG_NAME + ".hip")


def test_the_library_exports_the_batched_sampler(pkg):
    hip = _hip()
    names = hip.check_exports()                   # header == ctypes table == exported symbols
    raw = ctypes.CDLL(hip.SO_PATH)
    for name in NEW:
        assert name in names and name in hip._SIGS
        getattr(raw, name)


def test_a_null_context_is_an_argument_error(pkg):
    hip = _hip()
    L = hip.lib()
    assert L.gl3_forward_decode_batch_sample(None, None, None, None, 1, None, None, None, None) == hip.E_ARG
    assert L.gl3_get_sample_probs_row(None, 0, None) == hip.E_ARG
    assert L.gl3_sample_rows(None, None, 1, None, None, None, None) == hip.E_ARG


def test_the_plan_mirrors_the_three_entry_points(pkg):
    _hip()
    from importlib import import_module
    plan_mod = import_module(ge.PKG_NAME + ".plan")
    for name in ("forward_decode_batch_sample", "sample_probs_row", "sample_rows"):
        assert callable(getattr(plan_mod.HipMasterPlan, name))
