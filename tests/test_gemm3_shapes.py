"""The rule and the grid of tests/gemm3_shapes.py, checked without a GPU: the Python rule equals the library's own plan (gl3_debug_gemm3_plan:
g3_plan of csrc/gl3_prefill_gemm3.hip, what g3_dispatch launches) for every launch of every grid row and around every boundary, the tile
mapping hands every tile to exactly one workgroup, the grid covers every branch and needs every row, and the shapes are legal for gl3_create."""
import ctypes as C
import os
import subprocess
import sys

import pytest

import __graft_entry__ as ge
import gemm3_shapes as gs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ge.PKG_DIR, "csrc")
EPIS = ("store", "resid", "swiglu")


@pytest.fixture(scope="module")
def mods():
    if not os.path.exists(os.path.join(ge.PKG_DIR, "libgpullama_hip.so")):
        ge.build()
    ge.load_package()
    from importlib import import_module
    return import_module(ge.PKG_NAME + ".hip"), import_module(ge.PKG_NAME + ".plan")


def switches():
    """The process's switches as the library reads them (unset = default; atoi of the value otherwise)"""
    def num(name, dflt):
        v = os.environ.get(name)
        return dflt if v is None else int(v or 0)
    return dict(tall=num("GL3_PF_GEMM3_TALL", 0), tall_kb=num("GL3_PF_GEMM3_TALL_KB", 2), shape=num("GL3_PF_GEMM3_SHAPE", 0),
                qout=num("GL3_PF_GEMM3_QOUT", 1) != 0)


def boundary_sweep():
    """(epi, rows, ntok) on both sides of every branch: t128 511 / 512, t96 128 / 129 and 384 / 385, rows % 96, every NFR step, 64 / 65 tokens"""
    out = []
    for ntok in (1, 64, 65, 127, 128, 129, 256, 257, 384, 385, 512, 513, 640, 641, 1024, 1025):
        ntt = gs.ceil_div(ntok, 128)
        rows = set()
        for tiles in (511, 512, 513):                           # t128: the first row count of ceil(tiles / ntt) row tiles and the last
            rt = gs.ceil_div(tiles, ntt)
            rows |= {128 * (rt - 1) + 16, 128 * rt, 128 * rt + 16}
        for tiles in (128, 129, 130, 384, 385, 386):            # t96, on multiples of 96 and 16 rows beside them
            rt = gs.ceil_div(tiles, ntt)
            rows |= {96 * (rt - 1), 96 * rt, 96 * rt - 16, 96 * rt + 16, 96 * (rt + 1)}
        out += [(epi, r, ntok) for epi in ("store", "resid") for r in sorted(rows) if r > 0]
        hid = set()
        for a in range(4, 8):                                   # gate + up: around every row count at which a cost term steps
            for wg in (256, 512, 768):
                r = 32 * a * gs.ceil_div(wg, ntt)
                hid |= {r - 32, r, r + 32}
            r64 = 64 * gs.ceil_div(512, ntt)
            hid |= {r64 - 32, r64, r64 + 32, 2 * r64, 2 * r64 + 32}
        hid |= {8192, 8224, 10240, 10272, 12288, 12320, 14336, 14368, 16416, 20512, 24608, 28672, 31872}
        out += [("swiglu", r, ntok) for r in sorted(hid) if r > 0]
    return out


def test_the_rule_equals_the_library(mods):
    """Every launch of every grid row, and the boundary sweep, under this process's switches"""
    _, plan_mod = mods
    sw = switches()
    n = 0
    for name in gs.GRID:
        for proj, epi, rows, k, ntok, scaled in gs.launches(name):
            assert plan_mod.gemm3_plan(epi, rows, ntok) == gs.plan(epi, rows, ntok, **sw), (name, proj)
            n += 1
    assert n >= 4 * len(gs.GRID)
    sweep = boundary_sweep()
    assert len(sweep) > 1000
    for epi, rows, ntok in sweep:
        assert plan_mod.gemm3_plan(epi, rows, ntok) == gs.plan(epi, rows, ntok, **sw), (epi, rows, ntok)
    for epi in EPIS:                                            # and a plain scan of row counts
        for rows in range(16, 36000, 208):
            for ntok in (65, 129, 385, 641):
                assert plan_mod.gemm3_plan(epi, rows, ntok) == gs.plan(epi, rows, ntok, **sw), (epi, rows, ntok)


def test_the_sweep_crosses_every_boundary():
    """Under the defaults the sweep holds both sides of each branch of the rule"""
    seen = {(epi, gs.tile_name(epi, gs.plan(epi, r, n)), gs.plan(epi, r, n)["NFR"]) for epi, r, n in boundary_sweep()}
    for epi in ("store", "resid"):
        assert {(epi, t, 0) for t in ("64x128", "96x128", "128x128")} <= seen
    assert {("swiglu", "swiglu 128x128", 0)} | {("swiglu", "tall", a) for a in (5, 6, 7)} <= seen and ("swiglu", "tall", 4) not in seen
    assert gs.plan("store", 128 * 511 + 16, 128)["tile_rows"] == 128 and gs.plan("store", 128 * 511, 128)["tile_rows"] == 64      # t128 512 / 511
    assert gs.plan("resid", 128 * 255 + 16, 129)["tile_rows"] == 128 and gs.plan("resid", 128 * 255 + 16, 128)["tile_rows"] == 64  # 2 x 256 / 1 x 256
    assert gs.plan("resid", 3072, 512)["tile_rows"] == 64 and gs.plan("resid", 3168, 512)["tile_rows"] == 96                       # t96 128 / 132
    assert gs.plan("resid", 96 * 96, 512)["tile_rows"] == 96 and gs.plan("resid", 96 * 97, 512)["tile_rows"] == 64                 # t96 384 / 388
    assert gs.plan("resid", 3168 + 16, 512)["tile_rows"] == 64                                                                     # rows % 96
    assert [gs.tall_choice(h, 512) for h in (8192, 8224, 10240, 10272, 12288, 12320, 14336, 14368)] == [0, 5, 5, 6, 6, 7, 7, 0]
    assert [gs.tall_choice(h, 256) for h in (16384, 16416, 20512, 24608, 28704)] == [0, 5, 6, 7, 0]
    assert all(gs.tall_cost(h, n, 4) >= gs.tall_cost(h, n, 0) for h in range(32, 40000, 32) for n in (65, 129, 385, 513, 1025)), "NFR 4 never wins"


ENVS = [{"GL3_PF_GEMM3_TALL": "-1"}, {"GL3_PF_GEMM3_TALL": "4"}, {"GL3_PF_GEMM3_TALL_KB": "1"}, {"GL3_PF_GEMM3_TALL": "5", "GL3_PF_GEMM3_TALL_KB": "1"},
        {"GL3_PF_GEMM3_TALL_KB": "3"}, {"GL3_PF_GEMM3_SHAPE": "1"}, {"GL3_PF_GEMM3_SHAPE": "2"}, {"GL3_PF_GEMM3_SHAPE": "3"}, {"GL3_PF_GEMM3_SHAPE": "4"},
        {"GL3_PF_GEMM3_QOUT": "0"}]


@pytest.mark.parametrize("env", ENVS, ids=["-".join("%s=%s" % (k[13:].lower(), v) for k, v in e.items()) for e in ENVS])
def test_the_rule_equals_the_library_under_each_switch(env):
    """The switches are read once per process: the test above in a child process per environment"""
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-k", "test_the_rule_equals_the_library and not switch",
                          "-p", "no:cacheprovider"], capture_output=True, text=True, timeout=300, env=dict(os.environ, **env), cwd=ROOT)
    tail = out.stdout[-1500:] + out.stderr[-500:]
    assert out.returncode == 0, tail
    assert "1 passed" in out.stdout and "failed" not in out.stdout and "skipped" not in out.stdout, tail


def test_what_the_switches_do():
    """The Python rule under each switch, stated on shapes of the grid"""
    assert gs.plan("swiglu", 8224, 385, tall=-1)["kernel"] == gs.G3 and gs.plan("swiglu", 288, 65, tall=4) == dict(
        kernel=gs.G3T, tile_rows=128, tile_tok=128, KB=2, NFR=4, ntt=1, qout=1, nrt=3, grid=8)
    assert gs.plan("swiglu", 8224, 385, tall_kb=1)["KB"] == 1 and gs.plan("swiglu", 8224, 385, tall_kb=1)["qout"] == 0
    assert gs.plan("swiglu", 8224, 385, qout=False)["qout"] == 0 and gs.plan("swiglu", 8224, 385)["qout"] == 1
    assert gs.plan("swiglu", 8208, 385)["qout"] == 0                       # rows % 32: a result tile would not be one activation block
    assert gs.plan("resid", 160, 97, shape=4) == dict(kernel=gs.G3, tile_rows=64, tile_tok=64, KB=4, NFR=0, ntt=2, qout=0, nrt=3, grid=8)
    assert gs.plan("resid", 160, 97, shape=1)["tile_rows"] == 128 and gs.plan("resid", 160, 97, shape=2)["tile_rows"] == 96


def test_the_library_refuses_bad_arguments(mods):
    hip, _ = mods
    out = (C.c_int32 * 9)()
    f = hip.lib().gl3_debug_gemm3_plan
    assert f(0, 64, 65, out) == 0 and f(1, 64, 65, out) == 0 and f(2, 64, 65, out) == 0
    for epi, rows, ntok in ((3, 64, 65), (-1, 64, 65), (0, 0, 65), (0, 64, 0)):
        assert f(epi, rows, ntok, out) == hip.E_ARG, (epi, rows, ntok)
    assert f(0, 64, 65, None) == hip.E_ARG


@pytest.mark.parametrize("sw", [dict(), dict(tall=4), dict(tall=7, tall_kb=1), dict(tall=-1), dict(shape=1), dict(shape=2), dict(shape=4)],
                         ids=["default", "tall4", "tall7-kb1", "never-tall", "shape1", "shape2", "shape4"])
def test_every_tile_goes_to_exactly_one_workgroup(sw):
    for name in gs.GRID:
        for proj, epi, rows, k, ntok, scaled in gs.launches(name):
            pl = gs.plan(epi, rows, ntok, **sw)
            got = [t for t in gs.tiles(pl) if t is not None]
            assert sorted(got) == [(r, t) for r in range(pl["nrt"]) for t in range(pl["ntt"])], (name, proj)
            assert pl["grid"] % 8 == 0 and 0 <= pl["grid"] - pl["nrt"] * pl["ntt"] < 8 and gs.tiles(pl).count(None) == pl["grid"] - pl["nrt"] * pl["ntt"]
            assert pl["nrt"] * pl["tile_rows"] >= rows > (pl["nrt"] - 1) * pl["tile_rows"]
            assert pl["ntt"] * pl["tile_tok"] >= ntok > (pl["ntt"] - 1) * pl["tile_tok"]
            per_xcd = pl["grid"] // 8                      # an XCD's slots are consecutive tiles: the token tiles of a row tile stay together
            for b, t in enumerate(gs.tiles(pl)):
                assert t is None or t[0] * pl["ntt"] + t[1] == (b & 7) * per_xcd + (b >> 3)


def test_the_grid_reaches_what_the_issue_names():
    """The branch each row was chosen for, stated from the rule"""
    def of(name, proj):
        epi, rows, ntok = next((l[1], l[2], l[4]) for l in gs.launches(name) if l[0] == proj)
        return gs.plan(epi, rows, ntok)
    assert of("tall5-385", "gate+up") == dict(kernel=gs.G3T, tile_rows=160, tile_tok=128, KB=2, NFR=5, ntt=4, qout=1, nrt=52, grid=208)
    assert of("tall6-512", "gate+up") == dict(kernel=gs.G3T, tile_rows=192, tile_tok=128, KB=2, NFR=6, ntt=4, qout=1, nrt=54, grid=216)
    assert of("tall7-385", "gate+up") == dict(kernel=gs.G3T, tile_rows=224, tile_tok=128, KB=2, NFR=7, ntt=4, qout=1, nrt=55, grid=224)
    assert 8224 % 160 == 2 * 32 and 10272 % 192 == 3 * 32 and 12320 % 224 == 0
    assert of("tall-end-385", "gate+up") == dict(kernel=gs.G3, tile_rows=64, tile_tok=128, KB=2, NFR=0, ntt=4, qout=0, nrt=225, grid=904)
    for proj in ("wo", "down"):
        assert of("r96-385", proj) == dict(kernel=gs.G3, tile_rows=96, tile_tok=128, KB=4, NFR=0, ntt=4, qout=0, nrt=33, grid=136)
        assert of("r96-below-385", proj) == dict(kernel=gs.G3, tile_rows=64, tile_tok=128, KB=4, NFR=0, ntt=4, qout=0, nrt=48, grid=192)
        assert of("tails-97", proj) == dict(kernel=gs.G3, tile_rows=64, tile_tok=128, KB=4, NFR=0, ntt=1, qout=0, nrt=3, grid=8)
    assert of("tails-161", "gate+up") == dict(kernel=gs.G3, tile_rows=64, tile_tok=128, KB=2, NFR=0, ntt=2, qout=0, nrt=5, grid=16)
    assert of("s96-m65f65", "logits") == dict(kernel=gs.G3, tile_rows=96, tile_tok=128, KB=4, NFR=0, ntt=1, qout=0, nrt=129, grid=136)
    assert of("s96-m257f256", "logits")["tile_rows"] == 96 and of("s96-m257f257", "logits")["tile_rows"] == 64
    assert [l[0] for l in gs.launches("s96-m65f64")] == ["qkv", "wo", "gate+up", "down"]          # 64 output rows: not these kernels
    assert of("s128-m129f129", "logits") == dict(kernel=gs.G3, tile_rows=128, tile_tok=128, KB=2, NFR=0, ntt=2, qout=0, nrt=256, grid=512)
    assert of("s128-m129f128", "logits")["tile_rows"] == 64 and 32672 % 128 == 32
    assert of("s128-m161f161", "logits") == of("s128-m129f129", "logits") and gs.last_tile_tokens(161) == 33
    assert [l[0] for l in gs.launches("s96-m257f64")] == ["qkv", "wo", "gate+up", "down"] and of("s96-m257f65", "logits") == of("s96-m65f65", "logits")
    assert of("tall-end-512", "gate+up") == of("tall-end-385", "gate+up") and of("r96-below-512", "down") == of("r96-below-385", "down")
    # K stages: (stages, real blocks of the last) of qkv / gate + up / down
    ks = {c: (gs.stages(gs.CASES[c]["dim"], 4), gs.stages(gs.CASES[c]["dim"], 2), gs.stages(gs.CASES[c]["hidden"], 4)) for c in ("k1", "k2", "k3", "k4", "tails")}
    assert ks == {"k1": ((1, 1), (1, 1), (1, 3)), "k2": ((1, 3), (2, 1), (2, 2)), "k3": ((3, 4), (6, 2), (4, 4)), "k4": ((2, 3), (4, 1), (4, 1)),
                  "tails": ((2, 1), (3, 1), (3, 1))}
    assert gs.stages(gs.Q_DIM, 4) == (2, 4)


def test_the_grid_covers_every_branch_and_needs_every_row():
    names = sorted(gs.GRID)
    assert gs.missing(names) == []
    for drop in names:
        # "stale token slots" needs a longer and a shorter step of a case by construction, so it does not count here: every row has to
        # bring a tile shape, a tail, a K loop, a boundary of the choice or a logits stage that no other row does
        lost = [w for w in gs.missing([n for n in names if n != drop]) if w[0] != "stale token slots"]
        assert lost, "the grid covers the same without %s" % drop
    assert len(names) == 57 and set(gs.FORM_ROWS) <= set(names)
    assert gs.missing([]) == gs.wanted() and len(set(gs.wanted())) == len(gs.wanted())
    # every case runs a shorter step over the token slots of a longer one (the GPU test runs a case's steps longest first)
    for case in gs.CASES:
        assert len({gs.ntok_of(r["step"])[0] for r in gs.GRID.values() if r["case"] == case}) > 1, case


def test_the_form_rows_give_the_128x128_residual_tile_every_tail():
    """Under GL3_PF_GEMM3_SHAPE=1, the only way the 128 x 128 tile meets the residual epilogue (FORM_ROWS says why)"""
    tails = {"one token tile": set(), "several": set()}
    for name in gs.FORM_ROWS:
        for proj, epi, rows, k, ntok, scaled in gs.launches(name):
            pl = gs.plan(epi, rows, ntok, shape=1)
            if epi == "resid":
                assert gs.plan(epi, rows, ntok)["tile_rows"] != 128 and (pl["tile_rows"], pl["KB"]) == (128, 2)
                tails["one token tile" if pl["ntt"] == 1 else "several"].add(gs.last_tile_tokens(ntok))
    assert tails["one token tile"] >= {65, 97} and tails["one token tile"] | tails["several"] >= set(gs.TAILS)
    assert not any(gs.plan("resid", c["dim"], 512)["tile_rows"] == 128 for c in gs.CASES.values())
    assert gs.plan("resid", 10912, 641)["tile_rows"] == 128 and gs.plan("resid", 10912 - 32, 641)["tile_rows"] != 128 and gs.plan("resid", 10912, 640)["tile_rows"] != 128


def test_the_edge_value_cases_take_the_tall_kernel_and_the_96x128_tile_by_default(mods):
    _, plan_mod = mods
    got = {case: {l[0]: gs.plan(l[1], l[2], l[4]) for l in gs.edge_launches(case)} for case in gs.EDGE_CASES}
    assert got["edge-tall"]["gate+up"] == dict(kernel=gs.G3T, tile_rows=160, tile_tok=128, KB=2, NFR=5, ntt=4, qout=1, nrt=52, grid=208)
    assert got["edge-r96"]["wo"] == got["edge-r96"]["down"] == dict(kernel=gs.G3, tile_rows=96, tile_tok=128, KB=4, NFR=0, ntt=4, qout=0, nrt=33, grid=136)
    if not any(k.startswith("GL3_PF_GEMM3_") for k in os.environ):
        for case in gs.EDGE_CASES:
            for l in gs.edge_launches(case):
                assert plan_mod.gemm3_plan(l[1], l[2], l[4]) == got[case][l[0]], (case, l[0])
    for case, c in gs.EDGE_CASES.items():            # the edits of edge_models.py are laid out for 8 blocks or more of dim and of hidden
        assert c["dim"] // 32 >= 8 and c["hidden"] // 32 >= 8 and c["step"] % 128 == 1, case


@pytest.mark.parametrize("case", list(gs.EDGE_CASES))
def test_the_edge_value_cases_reach_every_block_class(case):
    """By the reference oracles alone (test_edge_models.survey, the first 12 tokens of the chunk): at these shapes too, the operand of every
    projection of every layer has an all-zero block, one whose f16 scale is subnormal and one with a scale above 1, and the operands of qkv,
    gate + up and down (hb: what the tall kernel's epilogue quantises) a block whose scale rounds to zero while its quants do not"""
    from test_edge_models import CONSUMERS, N_TOKENS, survey
    c = gs.EDGE_CASES[case]
    s = survey(c["cfg"], dim=c["dim"], hidden=c["hidden"], ctx=(c["step"] + 64 + 3) & ~3)
    assert s["finite"] and s["max_isum"] >= 400000 and s["min_prod"] < 2.0 ** -40
    assert s["toks"] == gs.edge_tokens(ge.load_package(), s["model"], c["step"])[:N_TOKENS]
    for l in range(gs.LAYERS):
        for cons in CONSUMERS:
            want = {"zero", "subnormal", "big"} | ({"scale0-quants"} if cons != "wo" else set())
            assert want <= s["classes"][(l, cons)], (case, l, cons, s["classes"][(l, cons)])


def test_the_constants_are_the_ones_in_the_kernel_sources():
    src = open(os.path.join(CSRC, "gl3_prefill_gemm3.hip")).read()
    assert "t128 >= 512 ? 1 : (rows % 96 == 0 && t96 > 128 && t96 <= 384) ? 2 : 3" in src
    assert "((ntt * ((rows + 63) / 64) + 511) / 512) * 8" in src and "((ntt * ((rows + 32 * nfr - 1) / (32 * nfr)) + 255) / 256) * 2 * nfr" in src
    assert "if (c < cost) { cost = c; best = nfr; }" in src and "p.grid = 8 * ((p.ntt * p.nrt + 7) / 8);" in src
    for h in ("gl3_prefill_gemm3.h", "gl3_prefill_gemm3t.h"):
        k = open(os.path.join(CSRC, h)).read()
        assert "per_xcd = (a.ntt * a.nrt + 7) >> 3;" in k and "J = (lin & 7) * per_xcd + (lin >> 3);" in k and "if (J >= ntt_g * a.nrt) return;" in k
    assert "constexpr int G3_RING = %d;" % gs.RING in open(os.path.join(CSRC, "gl3_prefill_gemm3.h")).read()
    hdr = open(os.path.join(ROOT, "include", "gpullama3_hip.h")).read()
    assert all(k in hdr for k in gs.KERNELS) and "gl3_debug_gemm3_plan" in hdr


def _create(hip, case, **over):
    """gl3_create on the case's description -> (code, message); without a device an accepted description ends in GL3_E_HIP"""
    c = gs.CASES[case]
    g = gs.GRANITE if c.get("granite") else dict(embedding_scale=1.0, attention_scale=0.0, residual_scale=1.0, logit_scale=1.0)
    d = hip.ModelDesc(C.sizeof(hip.ModelDesc), 3 if c.get("granite") else 0, c["dim"], c["hidden"], gs.LAYERS, gs.HEADS, gs.KV_HEADS, gs.HEAD_SIZE, c["vocab"],
                      gs.ctx_of(case), 1e-5, 8, c["batch"], 0, 0, 1, 0, 8, g["embedding_scale"], g["attention_scale"], g["residual_scale"], g["logit_scale"], 0, 0, 0)
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
    for case, c in gs.CASES.items():
        cfg = gs.case_config(pkg.synth, case)
        assert (cfg.n_layers, cfg.n_heads, cfg.n_kv_heads, cfg.head_size, cfg.q_dim) == (2, 8, 2, 32, 256), case
        deepest = max(gs.ntok_of(r["step"])[0] for r in gs.GRID.values() if r["case"] == case)
        assert cfg.ctx % 4 == 0 and cfg.ctx >= deepest + 64 and c["batch"] >= deepest > 64, case
        assert (cfg.residual_scale, cfg.logit_scale) == ((0.22, 8.0) if c.get("granite") else (1.0, 1.0))
        assert c["dim"] % 32 == 0 and c["hidden"] % 32 == 0 and c["vocab"] % 16 == 0, case
        code, msg = _create(hip, case)
        assert code in (0, hip.E_HIP), (case, code, msg)
    # dim 32 / hidden 32 are the smallest inner dimensions: one Q8_0 block
    code, msg = _create(hip, "k1", dim=16)
    assert code not in (0, hip.E_HIP), (code, msg)
