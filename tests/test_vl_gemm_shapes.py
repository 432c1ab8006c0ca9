"""The rule and the grid of tests/vl_gemm_shapes.py, checked without a GPU: the Python rule equals the library's own plan
(gl3_debug_vl_gemm_plan: vl_gemm_plan of csrc/gl3_prefill_vl.h, what launch_gemm_vl launches) for every launch of every grid row, the tile
mappings hand every tile to exactly one workgroup, the grid covers every branch and needs every row, and the shapes are legal for gl3_create."""
import ctypes as C
import os
import subprocess
import sys

import pytest

import __graft_entry__ as ge
import vl_gemm_shapes as vs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ge.PKG_DIR, "csrc")
ALL = [(name, kind) for name in vs.GRID for kind in vs.GRID[name]["kinds"]]


@pytest.fixture(scope="module")
def mods():
    if not os.path.exists(os.path.join(ge.PKG_DIR, "libgpullama_hip.so")):
        ge.build()
    ge.load_package()
    from importlib import import_module
    return import_module(ge.PKG_NAME + ".hip"), import_module(ge.PKG_NAME + ".plan")


def switches():
    """The process's switches as the library reads them (unset / empty = default; a flag is atoi(value) != 0)"""
    def flag(name, dflt):
        v = os.environ.get(name, "")
        return dflt if not v else int(v) != 0
    t = os.environ.get("GL3_VLQ_MFMA_MIN_TILES", "")
    return dict(mfma=flag("GL3_VLQ_MFMA", True), xcd_tokens=flag("GL3_VQM_XCD_TOKENS", True), min_tiles=int(t) if t and int(t) > 0 else vs.MIN_TILES)


def test_the_rule_equals_the_library(mods):
    """Every (grid row, weight type, projection), and a sweep of row and token counts around every threshold, under this process's switches"""
    hip, plan_mod = mods
    sw = switches()
    n = 0
    for name, kind in ALL:
        for proj, epi, rows, k, ntok, scaled in vs.launches(name):
            assert plan_mod.vl_gemm_plan(vs.KINDS[kind]["wtype"], vs.kind_flags(hip, kind), rows, ntok) == vs.plan(kind, rows, ntok, **sw), (name, kind, proj)
            n += 1
    assert n >= 5 * len(ALL)
    for kind in vs.KINDS:
        for rows in (8, 64, 72, 1536, 3072, 4096, 12224, 12288, 12296, 12304, 128256):
            for ntok in (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 448, 449, 511, 512, 513, 1024):
                assert plan_mod.vl_gemm_plan(vs.KINDS[kind]["wtype"], vs.kind_flags(hip, kind), rows, ntok) == vs.plan(kind, rows, ntok, **sw), (kind, rows, ntok)


@pytest.mark.parametrize("env", [{"GL3_VLQ_MFMA": "0"}, {"GL3_VQM_XCD_TOKENS": "0"}, {"GL3_VQM_OCC2": "1"}, {"GL3_VLQ_MFMA_MIN_TILES": "1"},
                                 {"GL3_VLQ_MFMA_MIN_TILES": "0"}, {"GL3_VLQ_MFMA_MIN_TILES": ""}],
                         ids=["valu-only", "vl_tile_of", "occ2", "min-tiles-1", "min-tiles-0-is-the-default", "min-tiles-empty-is-the-default"])
def test_the_rule_equals_the_library_under_each_switch(env):
    """The switches are read once per process: the test above in a child process per environment"""
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-k", "test_the_rule_equals_the_library and not switch",
                          "-p", "no:cacheprovider"], capture_output=True, text=True, timeout=300, env=dict(os.environ, **env), cwd=ROOT)
    tail = out.stdout[-1500:] + out.stderr[-500:]
    assert out.returncode == 0, tail
    assert "1 passed" in out.stdout and "failed" not in out.stdout and "skipped" not in out.stdout, tail


def test_the_library_refuses_what_does_not_batch_here(mods):
    hip, _ = mods
    out = (C.c_int32 * 7)()
    f = hip.lib().gl3_debug_vl_gemm_plan
    assert f(2, 0, 64, 17, out) == 0 and f(8, hip.FLAG_F32_ACTIVATION, 64, 17, out) == 0 and f(1, hip.FLAG_VECTOR_512, 64, 17, out) == 0
    for wt, flags, rows, ntok in ((8, 0, 64, 17), (2, hip.FLAG_F32_ACTIVATION, 64, 17), (2, hip.FLAG_SCALAR_DOT, 64, 17), (1, hip.FLAG_VECTOR_128, 64, 17),
                                  (2, hip.FLAG_VECTOR_512, 64, 17), (12, 0, 64, 17), (2, 0, 0, 17), (2, 0, 64, 0)):
        assert f(wt, flags, rows, ntok, out) == hip.E_ARG, (wt, flags, rows, ntok)
    assert f(2, 0, 64, 17, None) == hip.E_ARG


@pytest.mark.parametrize("sw", [dict(), dict(xcd_tokens=False), dict(min_tiles=1), dict(mfma=False)], ids=["default", "vl_tile_of", "min-tiles-1", "valu-only"])
def test_every_tile_goes_to_exactly_one_workgroup(sw):
    for name, kind in ALL:
        for proj, epi, rows, k, ntok, scaled in vs.launches(name):
            pl = vs.plan(kind, rows, ntok, **sw)
            got = [t for t in vs.tiles(pl) if t is not None]
            assert sorted(got) == [(r, t) for r in range(pl["nrt"]) for t in range(pl["ntt"])], (name, kind, proj)
            assert pl["grid"] % 8 == 0 and pl["nrt"] * 64 >= rows > (pl["nrt"] - 1) * 64
            tok = vs.VLQ_TOK if pl["kernel"] == vs.VALU else 64
            assert pl["ntt"] * tok >= ntok > (pl["ntt"] - 1) * tok
            if pl["xcd_tokens"]:                     # an XCD keeps a fixed token group and row part
                for b, t in enumerate(vs.tiles(pl)):
                    assert t is None or (t[1] % pl["G"] == (b & 7) % pl["G"] and t[0] % pl["P"] == (b & 7) // pl["G"])


def test_the_live_halves():
    assert [vs.live_halves(n, 0) for n in (1, 17, 32, 33, 64)] == [(True, False)] * 3 + [(True, True)] * 2
    assert vs.live_halves(193, 3) == (True, False) and vs.live_halves(225, 3) == (True, True) and vs.live_halves(513, 8) == (True, False)
    assert [vs.tail_class(n) for n in (193, 224, 225, 256, 17, 449, 512, 513, 65, 129)] == ["1", "32", "33", "64", "2..31", "1", "64", "1", "1", "1"]


def test_the_grid_reaches_what_the_issue_names():
    """The branch each row was chosen for, stated from the rule"""
    def of(name, proj, kind="q4v256"):
        rows, ntok = next((l[2], l[4]) for l in vs.launches(name) if l[0] == proj)
        return vs.plan(kind, rows, ntok)
    for kind in vs.BLOCK_KINDS:
        for proj in ("wo", "down"):
            assert of("resid-192", proj, kind) == dict(kernel=vs.VALU, nrt=48, ntt=12, grid=576, xcd_tokens=0, G=0, P=0)
            assert of("resid-193", proj, kind) == dict(kernel=vs.MFMA, nrt=48, ntt=4, grid=192, xcd_tokens=1, G=4, P=2)
            assert of("g8-448", proj, kind)["kernel"] == vs.VALU and of("g8-449", proj, kind) == dict(kernel=vs.MFMA, nrt=24, ntt=8, grid=192, xcd_tokens=1, G=8, P=1)
            assert of("g8-513", proj, kind) == dict(kernel=vs.MFMA, nrt=24, ntt=9, grid=384, xcd_tokens=1, G=8, P=1)
            assert of("store-193", proj, kind)["kernel"] == vs.VALU          # 8 row tiles beside gate / up
        for proj in ("qkv", "gate", "up"):
            assert of("resid-256", proj, kind)["kernel"] == vs.VALU          # K = 3072 on the VALU kernel in the same step
        for proj in ("gate", "up"):
            assert of("store-192", proj, kind)["kernel"] == vs.VALU and of("store-193", proj, kind) == dict(kernel=vs.MFMA, nrt=48, ntt=4, grid=192, xcd_tokens=1, G=4, P=2)
        assert of("rows-b16", "logits", kind) == dict(kernel=vs.VALU, nrt=193, ntt=1, grid=200, xcd_tokens=0, G=0, P=0)
        for s in ("b17", "b32", "b33", "b64"):
            assert of("rows-" + s, "logits", kind) == dict(kernel=vs.MFMA, nrt=193, ntt=1, grid=8 * 25, xcd_tokens=1, G=1, P=8)
        assert of("rows-m65", "logits", kind) == dict(kernel=vs.MFMA, nrt=193, ntt=2, grid=8 * 49, xcd_tokens=1, G=2, P=4)
        assert of("rows-m129", "logits", kind) == dict(kernel=vs.MFMA, nrt=193, ntt=3, grid=8 * 49 * 2, xcd_tokens=1, G=2, P=4)
        assert vs.tiles(of("rows-m129", "logits", kind)).count(None) == 8 * 49 * 2 - 193 * 3
    assert of("rows-b33", "logits", "f16v512") == dict(kernel=vs.KERNELS[1], nrt=193, ntt=1, grid=200, xcd_tokens=0, G=0, P=0)


def test_the_grid_covers_every_branch_and_needs_every_row():
    names = sorted(vs.GRID)
    assert vs.missing(names) == []
    for drop in names:
        assert vs.missing([n for n in names if n != drop]), "the grid covers the same without %s" % drop
    assert len(names) == 19 and set(vs.FORM_ROWS) <= set(names)
    for name in vs.FORM_ROWS:                        # the rows of the A/B switches take the matrix-pipe kernel by default
        assert any(vs.plan("q4v256", l[2], l[4])["kernel"] == vs.MFMA for l in vs.launches(name)), name
    assert vs.missing([]) == vs.wanted()


def test_the_constants_are_the_ones_in_the_kernel_sources():
    src = open(os.path.join(CSRC, "gl3_prefill_vl.h")).read()
    assert "constexpr int VLQ_TOK = %d;" % vs.VLQ_TOK in src and "VQM_ROWS = %d, VQM_TOK = %d," % (vs.TILE_ROWS, vs.VQM_TOK) in src
    assert "F16G_ROWS = %d, F16G_TOK = %d;" % (vs.TILE_ROWS, vs.F16G_TOK) in src and "constexpr int VQM_MIN_TILES = %d;" % vs.MIN_TILES in src
    assert "return ntt >= 8 ? 8 : ntt >= 4 ? 4 : ntt >= 2 ? 2 : 1;" in src
    assert "ntok > VLQ_TOK && sw.mfma && p.nrt * ((ntok + VQM_TOK - 1) / VQM_TOK) >= sw.min_tiles" in src
    hdr = open(os.path.join(ROOT, "include", "gpullama3_hip.h")).read()
    assert all(k in hdr for k in vs.KERNELS) and "GL3_VLQ_MFMA_MIN_TILES" in hdr


def _create(hip, case, kind, **over):
    """gl3_create on the case's description -> (code, message); without a device an accepted description ends in GL3_E_HIP"""
    c = vs.CASES[case]
    g = vs.GRANITE if c.get("granite") else dict(embedding_scale=1.0, attention_scale=0.0, residual_scale=1.0, logit_scale=1.0)
    d = hip.ModelDesc(C.sizeof(hip.ModelDesc), 3 if c.get("granite") else 0, c["dim"], c["hidden"], vs.LAYERS, vs.HEADS, vs.KV_HEADS, vs.HEAD_SIZE, c["vocab"],
                      vs.ctx_of(case), 1e-5, vs.KINDS[kind]["wtype"], c["batch"], 0, 0, 1, vs.kind_flags(hip, kind), 68 if c["mode"] == "rows" else 10,
                      g["embedding_scale"], g["attention_scale"], g["residual_scale"], g["logit_scale"], 0, 0, 0)
    for k, v in over.items():
        setattr(d, k, v)
    h = C.c_void_p()
    code = hip.lib().gl3_create(C.byref(d), C.byref(h))
    msg = (hip.lib().gl3_last_error(None) or b"").decode()
    if code == 0:
        hip.lib().gl3_destroy(h)
    return code, msg


def test_every_shape_is_legal(mods, pkg):
    hip, _ = mods
    assert pkg.synth.ARCH_GRANITE == 3 and pkg.synth.ARCH_LLAMA == 0
    for case, c in vs.CASES.items():
        cfg = vs.case_config(pkg.synth, case)
        assert (cfg.n_layers, cfg.n_heads, cfg.n_kv_heads, cfg.head_size, cfg.q_dim) == (2, 8, 2, 32, 256), case
        deepest = max(vs.ntok_of(r["step"]) for r in vs.GRID.values() if r["case"] == case)
        assert cfg.ctx % 4 == 0 and cfg.ctx >= deepest + 64 and c["batch"] >= deepest, case
        assert (cfg.residual_scale, cfg.logit_scale) == ((0.22, 8.0) if case == "resid-granite" else (1.0, 1.0))
        kinds = set(k for r in vs.GRID.values() if r["case"] == case for k in r["kinds"])
        for kind in kinds:
            step = vs.KINDS[kind]["step"]
            assert c["dim"] % step == 0 and c["hidden"] % step == 0 and vs.Q_DIM % step == 0, (case, kind)
            code, msg = _create(hip, case, kind)
            assert code in (0, hip.E_HIP), (case, kind, code, msg)
    # the vocabulary of "rows": 8-row granularity is refused, so the smallest legal count above 12288 that 64 does not divide is 12304
    assert vs.CASES["rows"]["vocab"] == 12304 and 12304 % 64 == 16
    for kind in vs.BLOCK_KINDS:
        code, msg = _create(hip, "rows", kind, vocab=12296)
        assert code == hip.E_UNSUPPORTED and "vocab/16" in msg, (kind, code, msg)
