"""What the inner-dimension grid (tests/k_shapes.py) covers and the rule it states, checked without a GPU; the limits against the library's
own answers (gl3_create refuses before it touches a device) and the thresholds against the kernel sources."""
import ctypes as C
import os
import re

import pytest

import __graft_entry__ as ge
import k_shapes as ks

CSRC = os.path.join(ge.PKG_DIR, "csrc")


def test_the_grid_covers_every_boundary_of_every_weight_type():
    """Per weight type the last legal multiple below 1024, 1024, 5120, the first legal multiple above 5120 and the named large dims; per copy
    of the sum-of-squares split both forms.  Dropping a row must fail."""
    names = sorted(ks.GRID)
    assert ks.missing(names) == []
    for drop in names:
        assert ks.missing([n for n in names if n != drop]), "the grid covers the same without %s" % drop
    assert len(names) == 41
    for kind, k in (("q8", 992), ("q8", 5152), ("f16v256", 960), ("f16v256", 5184), ("q4v256", 768), ("q4v256", 5376), ("q8f32", 896), ("q8f32", 5248),
                    ("f16s", 960), ("q4s", 5184), ("moe", 2080), ("q8h", 14368)):
        assert "%s-%d" % (kind, k) in ks.GRID
    for name, (kind, k, vocab) in ks.GRID.items():
        assert k % ks.KINDS[kind]["step"] == 0 and vocab % 16 == 0, name


def test_the_rule():
    assert [ks.sumsq_form(k) for k in (992, 1024, 5120, 5152)] == ["seq", "exact", "exact", "seq"]
    assert [ks.q8_rms_in_registers(k) for k in (5120, 5152)] == [True, False]
    assert [ks.q8_quant_in_registers(k) for k in (14336, 14368)] == [True, False]
    assert [ks.moe_router_in_registers(k) for k in (2048, 2080)] == [True, False]
    # F16 fuses inside the range whatever the row count; a K-split type only with more than 512 8-row groups, never into a residual epilogue
    assert ks.vl_fuse_rms(5120, 96, False) and not ks.vl_fuse_rms(5184, 96, False) and not ks.vl_fuse_rms(960, 96, False)
    assert not ks.vl_fuse_rms(5120, 4096, True) and ks.vl_fuse_rms(5120, ks.BIG_VOCAB, True) and not ks.vl_fuse_rms(5376, ks.BIG_VOCAB, True)
    assert ks.vl_fuse_rms(5120, 2052, True, swiglu=True) and not ks.vl_fuse_rms(5120, ks.BIG_VOCAB, False, resid=True)
    assert ks.nq_smem(9312) <= 64 * 1024 < ks.nq_smem(9344) and ks.nq_smem(1) == 7 + 320
    assert (ks.Q8_MAX_DIM, ks.Q8_MAX_HIDDEN, ks.NQ_MAX_K, ks.VL_MAX_K, ks.SCALAR_MAX_DIM, ks.MOE_MAX_DIM) == (12416, 31872, 23296, 16384, 23296, 4160)
    assert ks.nq_smem(ks.Q8_MAX_DIM) > 64 * 1024, "the largest Q8_0 dim needs the raised limit of pf_norm_quant_kernel"
    # which copies a case runs
    assert ks.sumsq_copies("f16v256-1024") == {("pf_f32", "exact"), ("vl", "exact")}
    assert ks.sumsq_copies("f16v256-5184") == {("pf_f32", "seq"), ("rmsnorm", "seq")}
    assert ks.sumsq_copies("q4v256-1024") == {("pf_f32", "exact"), ("rmsnorm", "exact")}
    assert ks.sumsq_copies("q4v256-5120") == {("pf_f32", "exact"), ("rmsnorm", "exact"), ("vl_ksplit", "exact")}
    assert ks.sumsq_copies("q8f32-5248") == {("pf_f32", "seq"), ("rmsnorm", "seq")}
    assert ks.sumsq_copies("moe-992") == {("q8t", "seq"), ("pf", "seq"), ("router", "seq")}
    assert ks.sumsq_copies("q8h-18944") == {("q8t", "seq"), ("pf", "seq")}          # dim 256


def test_every_case_is_a_config_of_the_issue_shape(pkg):
    for name, (kind, k, vocab) in ks.GRID.items():
        c = ks.case_config(pkg.synth, name)
        assert (c.n_layers, c.n_heads, c.n_kv_heads, c.head_size, c.ctx, c.vocab) == (2, 8, 2, 32, 96, vocab), name
        assert (c.dim, c.hidden) == ((256, k) if kind == "q8h" else (k, 256)), name
        assert (c.n_experts, c.n_experts_used, c.moe_hidden) == ((8, 2, 128) if kind == "moe" else (0, 0, 0)), name


def _sources():
    return {f: open(os.path.join(CSRC, f)).read() for f in ("gl3_decode_kernels.h", "gl3_prefill.hip", "gl3_rowlane_kernels.h",
                                                             "gl3_veclane_kernels.h", "gl3_moe_kernels.h", "gl3_seqsum.h", "gl3_api.hip")}


def test_the_thresholds_are_the_ones_in_the_kernel_sources():
    """The restated constants against the text of the kernels: the split is written five times with the same bounds."""
    src = _sources()
    assert "a.k >= %d && a.k <= %d" % (ks.SS_LO, ks.SS_HI) in src["gl3_decode_kernels.h"]
    for f in ("gl3_prefill.hip", "gl3_rowlane_kernels.h", "gl3_veclane_kernels.h", "gl3_moe_kernels.h"):
        assert "k >= %d && k <= %d" % (ks.SS_LO, ks.SS_HI) in src[f], f
    assert sum(len(re.findall(r"k >= \d+ && (?:a\.)?k <= \d+", s)) for s in src.values()) == 5
    assert "NXV = (PRO == PRO_RMS) ? %d : %d;" % (ks.Q8_RMS_QUADS, ks.Q8_QUANT_QUADS) in src["gl3_decode_kernels.h"]
    assert "constexpr int MOE_QJ = %d;" % ks.MOE_QJ in src["gl3_moe_kernels.h"] and "constexpr int MOE_RR = %d;" % ks.MOE_RR in src["gl3_moe_kernels.h"]
    assert "ss_scratch_bytes(int n) { return 128 + (size_t)3 * n; }" in src["gl3_seqsum.h"]
    # the 512-wavefront condition of the K-split types: vl_matvec_plan's (the launch code asks it and holds no copy)
    assert "constexpr int VQ_FUSE_MIN_WAVES = %d;" % (ks.KSPLIT_MIN_WAVES - 1) in src["gl3_veclane_kernels.h"]
    assert "!(ksplit_type && (long)ngroups * nm <= VQ_FUSE_MIN_WAVES)" in src["gl3_veclane_kernels.h"] and "ksplit_type" not in src["gl3_api.hip"]
    assert "GL3_LDS_MAX = 160 * 1024 - 256;" in src["gl3_api.hip"]
    for kern in ("pf_norm_quant_kernel<PQ_NORM>", "pf_norm_quant_kernel<PQ_NORM_F32>"):
        assert re.search(r"hipFuncSetAttribute\(\(const void\*\)%s, hipFuncAttributeMaxDynamicSharedMemorySize, 160 \* 1024 - 256\)" % re.escape(kern),
                         src["gl3_prefill.hip"]), kern


def _create(hip, name, **over):
    """gl3_create on the case's description -> (code, message); a plan that does get made (a machine with a GPU) is destroyed"""
    kind = ks.GRID[name][0]
    dim, hidden = ks.dims_of(name)
    moe = (5, ks.N_EXPERTS, 2, 128) if kind == "moe" else (0, 0, 0, 0)
    d = hip.ModelDesc(C.sizeof(hip.ModelDesc), moe[0], dim, hidden, ks.LAYERS, ks.HEADS, ks.KV_HEADS, ks.HEAD_SIZE, ks.GRID[name][2], ks.CTX, 1e-5,
                      ks.KINDS[kind]["wtype"], 65 if ks.KINDS[kind]["batched"] else 1, 0, 0, 1, ks.case_flags(hip, name), 1, 1.0, 0.0, 1.0, 1.0, *moe[1:])
    for k, v in over.items():
        setattr(d, k, v)
    h = C.c_void_p()
    code = hip.lib().gl3_create(C.byref(d), C.byref(h))
    msg = (hip.lib().gl3_last_error(None) or b"").decode()
    if code == 0:
        hip.lib().gl3_destroy(h)
    return code, msg


@pytest.fixture(scope="module")
def hip():
    if not os.path.exists(os.path.join(ge.PKG_DIR, "libgpullama_hip.so")):
        ge.build()
    ge.load_package()
    from importlib import import_module
    return import_module(ge.PKG_NAME + ".hip")


def test_the_limits_equal_the_librarys(hip):
    """The largest K of every LDS formula is accepted by gl3_create's checks (without a device the call then ends in GL3_E_HIP at
    hipSetDevice), the next legal step is refused with GL3_E_UNSUPPORTED and a message that names the dimension, and the bytes the
    message reports are the restated formula's."""
    for name in ("q8-%d" % ks.Q8_MAX_DIM, "q8h-%d" % ks.Q8_MAX_HIDDEN, "f16s-%d" % ks.SCALAR_MAX_DIM, "f16v256-%d" % ks.VL_MAX_K, "moe-%d" % ks.MOE_MAX_DIM):
        code, msg = _create(hip, name)
        assert code in (0, hip.E_HIP), (name, code, msg)
    formulas = {"q8": lambda k: ks.matvec_smem("rms", "swiglu", k), "q8h": lambda k: ks.matvec_smem("quant", "resid", k), "f16s": ks.rmsnorm_smem}
    assert len(ks.REFUSED) == 5
    for kind, field, value, names_it in ks.REFUSED:
        name = next(n for n in ks.GRID if ks.GRID[n][0] == kind)
        code, msg = _create(hip, name, **{field: value})
        assert code == hip.E_UNSUPPORTED and names_it in msg, (kind, field, value, code, msg)
        if kind in formulas:
            assert "needs %d bytes of LDS, the limit is %d" % (formulas[kind](value), ks.LDS_MAX) in msg, msg
    # the batched quantiser's own limit lies above every accepted Q8_0 dim: reached first only through the formula
    assert ks.NQ_MAX_K > ks.Q8_MAX_DIM and ks.nq_smem(ks.NQ_MAX_K + 32) > ks.LDS_MAX
    # wo: n_heads * head_size is named when it is the one that does not fit
    code, msg = _create(hip, "q8-992", n_heads=8 * 125, n_kv_heads=2 * 125)      # q_dim 32000 > 31872
    assert code == hip.E_UNSUPPORTED and "n_heads * head_size = 32000" in msg, (code, msg)
