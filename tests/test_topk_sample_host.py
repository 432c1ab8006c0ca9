"""CPU-side checks of the top-k / min-p / top-p sampler's C-ABI: the four names are declared, mirrored and exported with matching parameter
kinds, and np.cumsum on float32 — the restatement's sequential sum (tests/topk_ref.py) — is a strictly sequential f32 chain."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge

NAMES = ["gl3_sample_rows_topk", "gl3_forward_batch_sample_topk", "gl3_forward_decode_sample_topk", "gl3_get_topk_row"]


def _hip():
    if not os.path.exists(os.path.join(ge.PKG_DIR, "libgpullama_hip.so")):
        ge.build()
    ge.load_package()
    from importlib import import_module
    return import_module(ge.PKG_NAME + ".hip")


@pytest.mark.parametrize("name", NAMES)
def test_declared_mirrored_exported(pkg, name):
    hip = _hip()
    assert name in hip.check_exports() and name in hip._SIGS          # header == ctypes table == exported symbols
    hdr = open(os.path.join(ge.ROOT, "include", "gpullama3_hip.h")).read()
    params = re.search(r"GL3_API int32_t %s\((.*?)\);" % name, hdr, re.S).group(1).split(",")
    res, args = hip._SIGS[name]
    assert res is C.c_int32 and len(args) == len(params)
    for decl, kind in zip(params, args):
        pointer = "*" in decl or "[" in decl
        assert pointer == (kind in (C.c_void_p, C.POINTER(C.c_int32))), (name, decl)
        if not pointer:
            assert kind is (C.c_float if "float" in decl else C.c_int32), (name, decl)


def test_float32_cumsum_is_the_sequential_sum():
    x = (np.random.default_rng(3).random(1024) ** 8).astype(np.float32)
    run, chain = np.float32(0), []
    for v in x:
        run = np.float32(run + v)
        chain.append(run)
    assert np.array_equal(np.cumsum(x, dtype=np.float32), np.array(chain, np.float32))
