"""The rule and the grid of tests/matvec_shapes.py, checked without a GPU: the Python rule equals the library's own plan
(gl3_debug_matvec_plan: vl_matvec_plan of csrc/gl3_veclane_kernels.h, what launch_matvec launches) on every launch of every grid case and on
a sweep of rows and K; the K-split kernel's partition hands every chunk to exactly one (round, wavefront, slot) in chain order; its clamped
loads stay inside the matrix group and the activation vector; the grid covers every fact and needs every case; the shapes are legal."""
import ctypes as C
import os

import pytest

import __graft_entry__ as ge
import matvec_shapes as ms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ge.PKG_DIR, "csrc")
COMBOS = (("rms", "store"), ("rms", "swiglu"), ("quant", "resid"))      # what launch_matvec is called with
CBYTES = {"q4v256": 1152, "q8f32": 1088}                               # bytes of one VL chunk of an 8-row group


@pytest.fixture(scope="module")
def mods():
    if not os.path.exists(os.path.join(ge.PKG_DIR, "libgpullama_hip.so")):
        ge.build()
    ge.load_package()
    from importlib import import_module
    return import_module(ge.PKG_NAME + ".hip"), import_module(ge.PKG_NAME + ".plan")


def sweep_rows(kind):
    """the group thresholds +- one group (and the 512-wavefront condition of two matrices), a lone group, a large count"""
    base = [8, 96, 2040, 2048, 2056, 4088, 4096, 4104, 4112, 16384, 128256]
    return base if kind not in ms.SCALAR else [1, 63, 64, 65, 96, 4096, 128256]


def sweep_ks(kind):
    return range(ms.STEP[kind], 16384 + 1, ms.STEP[kind])


def test_the_rule_equals_the_library(mods):
    hip, plan_mod = mods
    n = 0
    for case, kind in ms.GRID:
        for proj, pro, epi, rows, k, _ in ms.launches(case, kind):
            got = plan_mod.matvec_plan(ms.KINDS[kind]["wtype"], ms.kind_flags(hip, kind), pro, epi, rows, k)
            assert got == ms.plan(kind, pro, epi, rows, k), (case, kind, proj)
            assert got["lds"] <= got["lds_cap"], (case, kind, proj)
            n += 1
    assert n == 5 * len(ms.GRID)
    out = (C.c_int32 * 12)()
    f = hip.lib().gl3_debug_matvec_plan
    names = hip.MATVEC_KERNELS
    for kind in ms.KINDS:
        wt, flags = ms.KINDS[kind]["wtype"], ms.kind_flags(hip, kind)
        for pro, epi in COMBOS:
            for rows in sweep_rows(kind):
                for k in sweep_ks(kind):
                    assert f(wt, flags, hip.MATVEC_PRO[pro], hip.GEMM3_EPI[epi], rows, k, out) == 0, (kind, pro, epi, rows, k)
                    want = ms.plan(kind, pro, epi, rows, k)
                    got = list(out)
                    assert [names[got[0]]] + got[1:] == [want[f_] for f_ in ("kernel", "rms_launch", "nw", "MAXW", "grid", "threads", "lds", "lds_cap",
                                                                               "nch", "nrounds", "rc", "RCM")], (kind, pro, epi, rows, k)
                    assert want["lds"] <= want["lds_cap"], (kind, pro, epi, rows, k)
    # the K-split kernel asks for more than the 64 KB default where rc rounds up past K (Q4_0, one matrix: the 8B down projection on a
    # tensor-parallel rank of at most 255 groups): gl3_create raises the limit of its instantiations, and the request stays inside it
    assert ms.VL_LDS_CAP == 64 * 1024 < ms.plan("q4v256", "quant", "resid", 512, 14336)["lds"] == 65792 <= ms.VQ_LDS_CAP


def test_the_library_refuses_what_does_not_launch_here(mods):
    hip, _ = mods
    out = (C.c_int32 * 12)()
    f = hip.lib().gl3_debug_matvec_plan
    assert f(2, 0, 0, 0, 64, 256, out) == 0 and f(8, hip.FLAG_F32_ACTIVATION, 1, 1, 64, 128, out) == 0 and f(1, hip.FLAG_VECTOR_512, 0, 2, 64, 64, out) == 0
    assert f(2, hip.FLAG_SCALAR_DOT, 0, 0, 64, 64, out) == 0
    for wt, flags, pro, epi, rows, k in ((8, 0, 0, 0, 64, 128), (2, hip.FLAG_F32_ACTIVATION, 0, 0, 64, 256), (8, hip.FLAG_F32_ACTIVATION | hip.FLAG_SCALAR_DOT, 0, 0, 64, 128),
                                         (1, hip.FLAG_VECTOR_128, 0, 0, 64, 64), (2, hip.FLAG_VECTOR_512, 0, 0, 64, 256), (1, hip.FLAG_VECTOR_512 | hip.FLAG_SCALAR_DOT, 0, 0, 64, 64),
                                         (12, 0, 0, 0, 64, 256), (2, 0, 2, 0, 64, 256), (2, 0, 0, 3, 64, 256), (2, 0, 0, 0, 0, 256), (2, 0, 0, 0, 64, 0),
                                         (2, 0, 0, 0, 64, 128), (8, hip.FLAG_F32_ACTIVATION, 0, 0, 64, 192), (1, 0, 0, 0, 64, 96), (2, 0, 0, 0, 64, 16640), (1, 0, 0, 0, 64, 16448)):
        assert f(wt, flags, pro, epi, rows, k, out) == hip.E_ARG, (wt, flags, pro, epi, rows, k)
    assert f(2, 0, 0, 0, 64, 256, None) == hip.E_ARG


def every_partition():
    """(kind, nm, nw, MAXW, k) over every K and every wavefront count the rule can pick for it, and the plan of each"""
    for kind in ms.KSPLIT:
        for epi in ("resid", "swiglu"):
            for k in sweep_ks(kind):
                seen = set()
                for rows in (8, 2040, 2048, 4088, 4096):
                    pl = ms.plan(kind, "quant", epi, rows, k)
                    if pl["nw"] not in seen:
                        seen.add(pl["nw"])
                        yield kind, 2 if epi == "swiglu" else 1, k, pl


def test_every_chunk_belongs_to_one_round_wavefront_and_slot():
    n = 0
    for kind, nm, k, pl in every_partition():
        nw, nch, rc, rcm, ce = pl["nw"], pl["nch"], pl["rc"], pl["RCM"], ms.CHUNK[kind]
        assert pl["MAXW"] == (16 if nw == 16 else 8) and nw in (4, 8, 16) and nch == k // ce
        assert 1 <= rc <= rcm == ms.round_chunks(kind, pl["MAXW"], nm), (kind, nm, k, pl)
        sl = ms.slots(pl)
        order = [c for _, _, c_lo, nc in sl for c in range(c_lo, c_lo + nc)]             # slot u of the wavefront = chunk c_lo + u
        assert order == list(range(nch)), (kind, nm, k, pl)
        assert sl[0][3] >= 1, "wavefront 0 of round 0 has no chunk: the hand-over would read an unwritten chain value"
        assert all(nc <= rc for _, _, _, nc in sl)
        # once a wavefront has no chunk, no later one of the chain has: the chain value in LDS is the last one written
        ncs = [nc for _, _, _, nc in sl]
        assert all(b == 0 for a, b in zip(ncs, ncs[1:]) if a == 0), (kind, nm, k, pl)
        # the staged slice of every wavefront fits the LDS requested, and the staging registers cover a full round
        assert nm * 64 * 4 + nw * rc * ce * 4 == pl["lds"] <= ms.VQ_LDS_CAP
        assert ms.x_quads(kind, rcm) * 256 >= rcm * ce
        n += 1
    assert n > 300


def test_the_clamped_loads_stay_inside_the_group_and_the_activation():
    for kind, nm, k, pl in every_partition():
        ce, nch, rcm = ms.CHUNK[kind], pl["nch"], pl["RCM"]
        xq = ms.x_quads(kind, rcm)
        gbytes = nch * CBYTES[kind]                          # vl_group_bytes: the group's chunks, nothing behind them belongs to it
        for r in range(pl["nrounds"]):
            for w in range(pl["nw"]):
                c_lo, nc, chunks, quads = ms.issue_reads(kind, pl, r, w, xq)
                assert 0 <= c_lo and nc >= 1 and c_lo + nc <= nch, (kind, nm, k, r, w)
                for c in chunks:
                    # 16 bytes per lane of the quants, then 16 (Q4_0) / 8 (Q8_0) bytes per row of the scales
                    last = c * CBYTES[kind] + 1024 + (16 * 7 + 16 if kind == "q4v256" else 8 * 7 + 8)
                    assert 0 <= c and last <= gbytes and last <= (c + 1) * CBYTES[kind], (kind, nm, k, r, w, c)
                assert min(quads) >= 0 and 4 * max(quads) + 4 <= k, (kind, nm, k, r, w)
                # the loads a live slot consumes are its own chunk's; the clamped rest repeats the wavefront's last chunk and is not summed
                own = ms.slots(pl)[r * pl["nw"] + w]
                assert chunks[:own[3]] == list(range(own[2], own[2] + own[3]))
                assert all(q == own[2] * (ce // 4) + i for i, q in enumerate(quads[:own[3] * (ce // 4)]))


def test_the_grid_covers_every_fact_and_needs_every_case():
    names = list(ms.CASES)
    assert ms.missing(names) == []
    assert ms.unneeded(names) == []
    assert ms.missing([]) == ms.wanted() and len(set(ms.wanted())) == len(ms.wanted())
    assert set(ms.EAGER) <= set(names) and set(ms.EDGE) <= set(names)


def test_the_grid_reaches_what_the_issue_names():
    def of(case, kind, proj):
        return next(ms.plan(kind, l[1], l[2], l[3], l[4]) for l in ms.launches(case, kind) if l[0] == proj)

    def ncs(pl):
        return [s[3] for s in ms.slots(pl)]
    a = of("A", "q4v256", "down")
    assert (a["nw"], a["nch"], ncs(a)) == (4, 1, [1, 0, 0, 0]) and ncs(of("A", "q8f32", "wo")) == [1, 1, 0, 0]
    b = of("B", "q4v256", "down")
    assert (b["nw"], b["MAXW"], b["nch"], b["rc"], ncs(b)) == (8, 8, 33, 5, [5] * 6 + [3, 0])
    assert of("B-at", "q4v256", "down")["nw"] == 4 and ncs(of("B-at", "q4v256", "down")) == [8] * 4 and ncs(of("B-at", "q8f32", "down")) == [12] * 4
    c = of("C", "q8f32", "down")
    assert (c["nw"], c["nrounds"], c["rc"], ncs(c)) == (8, 2, 7, [7] * 14 + [0, 0])
    d4, d8 = of("D", "q4v256", "down"), of("D", "q8f32", "down")
    assert (d4["nw"], d4["MAXW"], d4["rc"], ncs(d4)) == (16, 16, 4, [4] * 12 + [1, 0, 0, 0]) and (d8["nrounds"], d8["rc"]) == (2, 4)
    e4, e8 = of("E", "q4v256", "gate/up"), of("E", "q8f32", "gate/up")
    assert (e4["nw"], e4["rms_launch"], ncs(e4)) == (16, 1, [2] * 16 + [1] + [0] * 15) and ncs(e8) == [2] * 25 + [0] * 7
    assert ncs(of("E8", "q4v256", "gate/up")) == [3] * 11 + [0] * 5 and of("E8", "q4v256", "gate/up")["MAXW"] == 8
    assert ncs(of("G-above", "q4v256", "down")) == [2, 2, 2, 2, 1, 0, 0, 0]
    assert of("B", "q4v256", "gate/up")["kernel"] == ms.VL_RMS and of("B", "q4v256", "logits")["grid"] == 129
    assert of("A", "q4v256", "logits")["kernel"] == ms.VLQ and of("A", "q4v256", "logits")["rms_launch"] == 1
    assert of("V-in", "f16v512", "logits")["kernel"] == ms.VL_RMS and of("V-above", "f16v256", "logits") == dict(
        kernel=ms.VL, rms_launch=1, nw=2, MAXW=0, grid=6, threads=128, lds=5184 * 4, lds_cap=65536, nch=0, nrounds=0, rc=0, RCM=0)
    assert of("R", "q4s", "logits")["grid"] == 2 and of("R", "f16s", "gate/up")["kernel"] == ms.RL


def test_the_constants_are_the_ones_in_the_kernel_sources():
    src = open(os.path.join(CSRC, "gl3_veclane_kernels.h")).read()
    assert "constexpr int VL_WAVES = %d;" % ms.VL_WAVES in src and "constexpr int VL_RMS_WAVES = %d;" % ms.VL_RMS_WAVES in src
    assert "constexpr int VQ_FUSE_MIN_WAVES = %d;" % ms.FUSE_MIN_WAVES in src
    assert "constexpr size_t VQ_LDS_MAX = 2 * 64 * 4 + (size_t)(16384 + 16 * 256) * 4;" in src and ms.VQ_LDS_CAP == 82432
    assert "return (WT == WT_Q4_0 ? 8 : 12) / (MAXW == 16 ? 2 : 1) / nm;" in src
    assert "while (nw < 16 && (long)ngroups * nw < 2048) nw *= 2;" in src and "while (nw > 4 && nch < nw) nw /= 2;" in src
    assert "return k >= %d && k <= %d && (k & 3) == 0;" % (ms.ks.SS_LO, ms.ks.SS_HI) in src
    # one partition: the kernel, the LDS request and the plan ask the same helpers, and nobody restates them
    assert src.count("(nch + cap - 1) / cap") == 1 and src.count("(nch + turns - 1) / turns") == 1 and "- 1) / (" not in src
    assert "const int nrounds = vq_rounds(VQ_WAVES * RCM, nch);" in src and "const int rc = vq_rc(VQ_WAVES * nrounds, nch);" in src
    assert "return {nrounds, vq_rc(nw * nrounds, nch)};" in src and "p.smem = vq_smem_bytes(wt, nm, p.waves, p.rc);" in src
    rl = open(os.path.join(CSRC, "gl3_rowlane_kernels.h")).read()
    assert "RL_PITCH = %d, RL_NP = %d," % (ms.RL_PITCH, ms.RL_WAVES - 1) in rl
    api = open(os.path.join(CSRC, "gl3_api.hip")).read()
    assert api.count("hipFuncAttributeMaxDynamicSharedMemorySize, (int)VQ_LDS_MAX") == 2
    assert "vl_matvec_plan(ctx->d.weight_type, ctx->d.flags, pro, epi, w.rows, w.k)" in api and "vq_waves" not in api and "vl_rms_fusable" not in api
    hdr = open(os.path.join(ROOT, "include", "gpullama3_hip.h")).read()
    assert "gl3_debug_matvec_plan" in hdr and all(k.split("<")[0] in hdr for k in ms.KINDS and (ms.RL, ms.VL, ms.VLQ))


def test_every_shape_is_legal(mods, pkg):
    """gl3_create on every case's description: without a device an accepted description ends in GL3_E_HIP"""
    hip, _ = mods
    for case, kind in ms.GRID:
        cfg = ms.case_config(pkg.synth, case, kind)
        d = ms.dims(case, kind)
        assert (cfg.n_layers, cfg.head_size, cfg.q_dim, cfg.ctx) == (1, 32, d["q_dim"], ms.CTX) and cfg.n_heads % cfg.n_kv_heads == 0, (case, kind)
        g = ms.GRANITE if ms.CASES[case].get("granite") else dict(embedding_scale=1.0, attention_scale=0.0, residual_scale=1.0, logit_scale=1.0)
        desc = hip.ModelDesc(C.sizeof(hip.ModelDesc), cfg.arch, cfg.dim, cfg.hidden, 1, cfg.n_heads, cfg.n_kv_heads, 32, cfg.vocab, cfg.ctx, 1e-5,
                             ms.KINDS[kind]["wtype"], 1, 0, 0, 1, ms.kind_flags(hip, kind), 1, g["embedding_scale"], g["attention_scale"], g["residual_scale"],
                             g["logit_scale"], 0, 0, 0)
        h = C.c_void_p()
        code = hip.lib().gl3_create(C.byref(desc), C.byref(h))
        msg = (hip.lib().gl3_last_error(None) or b"").decode()
        if code == 0:
            hip.lib().gl3_destroy(h)
        assert code in (0, hip.E_HIP), (case, kind, code, msg)
