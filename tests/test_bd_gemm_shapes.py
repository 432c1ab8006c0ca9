"""The rule and the grid of tests/bd_gemm_shapes.py, checked without a GPU: the Python rule equals the library's own plan
(gl3_debug_bd_gemm_plan: bd_gemm_plan of csrc/gl3_bd_gemm.h, what launch_gemm launches, and the placement functions the kernel itself
calls) on every launch of every grid step, for every token count and around every boundary; every (unit, token tile) goes to exactly one
workgroup; the grid covers every requirement and needs every case; the rings' reads past a strip and past the operands stay inside the
slack the library allocates; the shapes are legal for gl3_create."""
import ctypes as C
import os
import re

import pytest

import __graft_entry__ as ge
import bd_gemm_shapes as bs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ge.PKG_DIR, "csrc")


@pytest.fixture(scope="module")
def mods():
    if not os.path.exists(os.path.join(ge.PKG_DIR, "libgpullama_hip.so")):
        ge.build()
    ge.load_package()
    from importlib import import_module
    return import_module(ge.PKG_NAME + ".hip"), import_module(ge.PKG_NAME + ".plan")


def all_launches():
    """(case, form, n, projection, epilogue, rows, K, ntok, qout) of every bdw_gemm_kernel launch of the grid, each distinct one once"""
    seen, out = set(), []
    for case in bs.CASES:
        for form, n in bs.steps_of(case):
            for l in bs.launches(case, form, n):
                if (case,) + l not in seen:
                    seen.add((case,) + l)
                    out.append((case, form, n) + l)
    return out


def test_the_rule_equals_the_library_on_every_launch_of_the_grid(mods):
    _, plan_mod = mods
    ls = all_launches()
    assert len(ls) > 5 * len(bs.CASES) and {l[3] for l in ls} == {"qkv", "wo", "gate+up", "down", "logits"}
    for case, form, n, proj, epi, rows, k, ntok, q in ls:
        want = bs.plan(epi, rows, k, ntok, q)
        assert plan_mod.bd_gemm_plan(epi, rows, k, ntok, q) == want, (case, form, n, proj)
        for wg in sorted({0, 7, 8, want["grid"] // 2, want["grid"] - 9, want["grid"] - 1, want["grid"]}):      # the last: outside the grid
            assert plan_mod.bd_gemm_plan(epi, rows, k, ntok, q, wg)["place"] == bs.plan(epi, rows, k, ntok, q, wg)["place"], (case, proj, wg)


MATRICES = [(384, 992), (272, 2112), (544, 32)]          # rows x K: 24 / 17 strips and 17 strip pairs; K with a ragged tile in the last slot, of two trips, of one block


def test_the_rule_equals_the_library_for_every_token_count(mods):
    """ntok 1 .. 64 on three matrix shapes, every epilogue and both gate + up forms, every workgroup id of the grid; and one step on either
    side of every boundary: the token tiles at 16 k, the operand layout at 32 | 33, the kernel at 64 | 65 (65: not this kernel)"""
    _, plan_mod = mods
    for rows, k in MATRICES:
        for epi, q in (("store", False), ("resid", False), ("swiglu", False), ("swiglu", True)):
            for ntok in range(1, 67):
                want = bs.plan(epi, rows, k, ntok, q)
                assert plan_mod.bd_gemm_plan(epi, rows, k, ntok, q) == want, (rows, k, epi, q, ntok)
                if epi != "resid" and ntok in (1, 16, 17, 33, 64):
                    for wg in range(want["grid"] + 1):
                        assert plan_mod.bd_gemm_plan(epi, rows, k, ntok, q, wg)["place"] == bs.plan(epi, rows, k, ntok, q, wg)["place"], (rows, epi, q, ntok, wg)
    p = {n: plan_mod.bd_gemm_plan("store", 384, 992, n) for n in (15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65)}
    assert [p[n]["ntt"] for n in (15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64)] == [1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4]
    assert [p[n]["ts"] for n in (31, 32, 33, 63, 64, 65)] == [32, 32, 64, 64, 64, 0]
    assert p[65] == dict(ts=0, DA=0, qout=0, threads=0, ntt=0, units=0, grid=0, ntiles=0, trips=0, partial=0, place=None)
    assert p[64]["grid"] == 24 * 4 and plan_mod.bd_gemm_plan("swiglu", 544, 992, 64, True)["grid"] == 24 * 4      # 17 pairs pad to 24


def test_the_library_refuses_bad_arguments(mods):
    hip, _ = mods
    out = (C.c_int32 * 12)()
    f = hip.lib().gl3_debug_bd_gemm_plan
    assert [f(e, 64, 64, 5, 0, 0, out) for e in (0, 1, 2)] == [0, 0, 0]
    for epi, rows, k, ntok in ((3, 64, 64, 5), (-1, 64, 64, 5), (0, 0, 64, 5), (0, 64, 0, 5), (0, 64, 48, 5), (0, 64, 64, 0)):
        assert f(epi, rows, k, ntok, 0, 0, out) == hip.E_ARG, (epi, rows, k, ntok)
    assert f(0, 64, 64, 5, 0, 0, None) == hip.E_ARG


def test_every_unit_and_token_tile_goes_to_exactly_one_workgroup():
    """Over all workgroup ids of every launch of the grid: each (unit, token tile) once, every other id exits, the token tiles of a unit
    sit 8 ids apart (same id % 8: one XCD and its L2)"""
    for case, form, n, proj, epi, rows, k, ntok, q in all_launches():
        pl = bs.plan(epi, rows, k, ntok, q)
        at = [bs.place(wg, pl["ntt"], pl["units"]) for wg in range(pl["grid"])]
        live = [a for a in at if a is not None]
        assert sorted(live) == [(u, h) for u in range(pl["units"]) for h in range(pl["ntt"])], (case, form, n, proj)
        assert at.count(None) == pl["grid"] - pl["units"] * pl["ntt"] and pl["grid"] % 8 == 0 and 0 <= pl["grid"] // pl["ntt"] - pl["units"] < 8
        where = {a: wg for wg, a in enumerate(at) if a is not None}
        for u in range(pl["units"]):
            ids = [where[(u, h)] for h in range(pl["ntt"])]
            assert [b - a for a, b in zip(ids, ids[1:])] == [8] * (pl["ntt"] - 1) and len({i % 8 for i in ids}) == 1, (case, proj, u)
        assert pl["units"] * (32 if pl["qout"] else 16) >= rows > (pl["units"] - 1) * (32 if pl["qout"] else 16)
        assert pl["ntt"] * 16 >= ntok > (pl["ntt"] - 1) * 16


def test_the_grid_covers_every_requirement_and_needs_every_case():
    cases = list(bs.CASES)
    assert bs.missing(cases) == []
    assert bs.missing([]) == bs.wanted(()) and len(set(bs.wanted())) == len(bs.wanted())
    for drop in cases:
        lost = bs.missing([c for c in cases if c != drop])
        assert lost, "the grid covers the same without %s" % drop
    # what each case was chosen for, stated from the rule
    walk = {c: (bs.k_walk(v["dim"], 4), bs.k_walk(v["dim"], 8), bs.k_walk(v["hidden"], 8)) for c, v in bs.CASES.items()}
    assert [walk[c][0]["nb"] for c in ("k1", "k2", "k3", "k4")] == [1, 2, 3, 4]
    assert walk["k12"][0]["ntiles"] == 3 and walk["k12"][2]["ntiles"] == 7
    assert [(w["trips"], w["partial"]) for w in (walk["k16"][0], walk["k16"][2])] == [(1, 0), (1, 0)]
    assert [(walk[c][0]["ragged"], walk[c][0]["partial"], walk[c][2]["ragged"], walk[c][2]["partial"]) for c in ("k17", "k18", "k19")] == [(1, 1, 1, 1), (2, 1, 2, 1), (3, 1, 3, 1)]
    assert (walk["k31"][0]["trips"], walk["k31"][0]["partial"], walk["k31"][1]["trips"], walk["k31"][1]["partial"], walk["k31"][1]["ragged"]) == (1, 4, 0, 8, 3)
    assert (walk["k66"][0]["trips"], walk["k66"][0]["partial"], walk["k66"][1]["trips"], walk["k66"][1]["partial"], walk["k66"][1]["ntiles"]) == (4, 1, 2, 1, 17)
    assert bs.k_walk(bs.Q_DIM, 8) == dict(nb=8, nfull=2, ntiles=2, trips=0, partial=2, ragged=0)          # wo, in every case
    # the steps: every count in every form on the case with a ragged tile in the last slot, 32 | 33 and the three stale orders on every case
    for c in cases:
        steps = bs.steps_of(c)
        assert [n for f, n in steps if f == "chunk"][:7] == list(bs.STALE_ORDER), c
        for kind in ("chunk", "batch", "mixed"):
            got = {n for f, n in steps if f.startswith(kind)}
            assert got >= ({32, 33, 64} if not bs.CASES[c].get("every_count") else set(bs.COUNTS)), (c, kind)
    assert bs.outputs_of("mixed", 33) == 3 and bs.tslots(33) == 64 and bs.tslots(3) == 32 and bs.mixed_runs(33) == (1, [16, 16])
    assert bs.outputs_of("mixed-all", 32) == 32 and bs.outputs_of("mixed-all", 49) == 49
    assert all(sum(bs.mixed_runs(n)[1]) + bs.mixed_runs(n)[0] == n for n in range(1, 65))
    # the quantising form on one rank by default, the plain SwiGLU form on two ranks and under GL3_NO_FUSED_QUANT
    assert bs.fuse_q(33, 512) and not bs.fuse_q(33, 512, ranks=2) and not bs.fuse_q(33, 512, no_fused_quant=True) and not bs.fuse_q(65, 512)
    tp = {l[0]: l for l in bs.launches(bs.TP_CASE, "chunk", 33, ranks=2)}
    assert tp["wo"][2] == tp["down"][2] == 48 and bs.plan("resid", 48, 256, 33)["units"] == 3 and tp["gate+up"][5] is False


def test_the_rings_stay_inside_the_slack_the_library_allocates():
    """bdw_gemm_kernel guards no load: per launch of the grid, the furthest byte its rings read past the last strip of the matrix and past
    the operand buffers, against GL3_TAIL_PAD (csrc/gl3_ctx.h) and the sizes gl3_prefill_init allocates (read from the sources)."""
    ctx_h = open(os.path.join(CSRC, "gl3_ctx.h")).read()
    pad = eval(re.search(r"constexpr size_t GL3_TAIL_PAD = ([0-9 *]+);", ctx_h).group(1))
    pf = open(os.path.join(CSRC, "gl3_prefill.hip")).read()
    api = open(os.path.join(CSRC, "gl3_api.hip")).read()
    assert "hipMalloc((void**)&m.w, m.bytes() + GL3_TAIL_PAD)" in api
    assert "const size_t xq_bytes = MQP * (p->maxk + 4 * 32) + GL3_TAIL_PAD;" in pf and "const size_t xs_bytes = MQ * (p->maxk / 32) * 4;" in pf
    assert "hipMalloc((void**)&p->XS, xs_bytes + GL3_TAIL_PAD)" in pf and "const size_t MQ = M < BD_TS_MAX ? BD_TS_MAX : M;" in pf
    assert "hipMalloc((void**)&p->XQb, (size_t)BD_TS_MAX * p->maxk + GL3_TAIL_PAD)" in pf
    assert "hipMalloc((void**)&p->XSb, (size_t)BD_TS_MAX * (p->maxk / 32) * 4 + GL3_TAIL_PAD)" in pf
    assert "constexpr int TILE_BYTES = %d;" % bs.TILE_BYTES in open(os.path.join(CSRC, "gl3_decode_kernels.h")).read()
    worst = dict(w=0, xq=0, xs=0)
    for case, form, n, proj, epi, rows, k, ntok, q in all_launches():
        pl = bs.plan(epi, rows, k, ntok, q)
        reach, maxk = bs.ring_reach(k, pl["DA"], pl["ts"]), bs.maxk_of(case)
        strip = pl["ntiles"] * bs.TILE_BYTES
        assert reach["w"] - strip <= pad, (case, proj)                      # the last strip: everything past it is the matrix's slack
        second = proj == "down" and bs.fuse_q(n, bs.CASES[case]["hidden"])  # XQb / XSb, always 64 slots; else XQ / XS of at least 64 (128) slots
        xq_alloc = 64 * maxk + pad if second else 128 * (maxk + 128) + pad
        xs_alloc = 64 * (maxk // 32) * 4 + pad
        assert reach["xq"] <= xq_alloc and reach["xs"] <= xs_alloc, (case, proj, reach)
        worst = {key: max(worst[key], reach[key] - (strip if key == "w" else 0)) for key in worst}
    assert worst["w"] == 8 * bs.TILE_BYTES + 128 and worst["w"] < pad       # DA tiles and one scale header past a strip


def test_the_constants_are_the_ones_in_the_kernel_sources():
    h = open(os.path.join(CSRC, "gl3_bd_gemm.h")).read()
    assert "constexpr int BD_TS = %d, BD_TS_MAX = %d;" % (bs.BD_TS, bs.BD_TS_MAX) in h
    assert "return (id >> 3) % ntg;" in h and "return (id / (8 * ntg)) * 8 + (id & 7);" in h and "return ((strips + 7) / 8) * 8 * nt;" in h
    assert "bdw_place_tile(blockIdx.x, NTG)" in h and "bdw_place_unit(blockIdx.x, NTG)" in h          # the kernel calls what the export calls
    assert "const int nfull = a.nb >> 2;" in h and "for (; base + DA <= nfull; base += DA)" in h and "if (base < ntiles)" in h
    pf = open(os.path.join(CSRC, "gl3_prefill.hip")).read()
    assert "const BdGemmPlan pl = bd_gemm_plan(EPI, w.rows, w.k, ntok, quantised_out);" in pf
    assert "bdw_gemm_kernel<EPI, 4, 2, true, TS_>" in pf and "bdw_gemm_kernel<EPI, 4, 2, false, TS_>" in pf and "bdw_gemm_kernel<EPI, 8, 2, false, TS_>" in pf
    assert "pf_quant<PQ_NORM>(ctx, src, dim, src_cc, ctx->out_norm, rows, pf_operand(p, rows));" in pf      # the logits stage: the TS of its output rows
    assert "gl3_debug_bd_gemm_plan" in open(os.path.join(ROOT, "include", "gpullama3_hip.h")).read()


def _create(hip, case, **over):
    """gl3_create on the case's description -> (code, message); without a device an accepted description ends in GL3_E_HIP"""
    c = bs.CASES[case]
    g = bs.GRANITE if c.get("granite") else dict(embedding_scale=1.0, attention_scale=0.0, residual_scale=1.0, logit_scale=1.0)
    d = hip.ModelDesc(C.sizeof(hip.ModelDesc), 3 if c.get("granite") else 0, c["dim"], c["hidden"], bs.LAYERS, bs.HEADS, bs.KV_HEADS, bs.HEAD_SIZE, c["vocab"],
                      bs.CTX, 1e-5, 8, 65, 0, 0, 1, 0, 64, g["embedding_scale"], g["attention_scale"], g["residual_scale"], g["logit_scale"], 0, 0, 0)
    for k, v in over.items():
        setattr(d, k, v)
    h = C.c_void_p()
    code = hip.lib().gl3_create(C.byref(d), C.byref(h))
    msg = (hip.lib().gl3_last_error(None) or b"").decode()
    if code == 0:
        hip.lib().gl3_destroy(h)
    return code, msg


def test_every_shape_is_legal_and_no_row_count_is_off_16(mods, pkg):
    hip, _ = mods
    for case, c in bs.CASES.items():
        cfg = bs.case_config(pkg.synth, case)
        assert (cfg.n_layers, cfg.n_heads, cfg.n_kv_heads, cfg.head_size, cfg.q_dim, cfg.ctx) == (2, 8, 2, 32, 256, 96), case
        assert (cfg.residual_scale, cfg.logit_scale) == ((0.22, 8.0) if c.get("granite") else (1.0, 1.0))
        code, msg = _create(hip, case)
        assert code in (0, hip.E_HIP), (case, code, msg)
    # the rule's statement on rows: nothing gl3_create accepts has a Q8_0 row count that 16 does not divide
    for field, value in (("dim", 48), ("hidden", 48), ("hidden", 16), ("vocab", 24), ("vocab", 8)):
        code, msg = _create(hip, "k3", **{field: value})
        assert code not in (0, hip.E_HIP), (field, value, code, msg)
    code, msg = _create(hip, "k3", tp_size=2)               # dim / 2 = 48: accepted on two ranks
    assert code in (0, hip.E_HIP), (code, msg)
