"""The Q8_0 GEMM of a step of at most 64 rows (bdw_gemm_kernel) at every form of its K walk, of its grid and of its token tiles: the grid of
tests/bd_gemm_shapes.py, bit for bit (np.array_equal on f32, no tolerance anywhere) against the CPU oracle.

What a case reaches follows from the rule (bd_gemm_shapes.py restates it, tests/test_bd_gemm_shapes.py holds it to the library):
    k1 .. k4        K of one tile of 1 .. 4 blocks at both ring depths; 1, 7, 8, 9 strip pairs of the quantising gate + up form and strips of
                    the logits launch (the grid pads to 8 units, the surplus workgroups exit)
    k12 / k16       DA - 1 tiles; exactly DA full tiles (one full trip, no partial one); 16 and 17 strips on the logits launch
    k17 .. k19      DA full tiles and a ragged tile of 1, 2, 3 blocks alone in the partial trip; k17 is Granite's (out_scale != 1)
    k31             a ragged tile in the last slot of the partial trip (dim 992); EVERY token count 1 .. 64 at a 16-token tile edge, in every form
    k66             two full trips and a partial one (dim 2112); 17 strip pairs
Chunks: one plan per case takes its chunk sizes in the order of bd_gemm_shapes.STALE_ORDER (65, 64, 32, 64, 33, 64, 17, then the other
counts, longest first), each into a fresh sequence from position 0, so that every step runs over the slots a longer one (and the chunk-major
layout of the 65-token step) left behind; one oracle walk of 65 tokens serves them all.  Compared: x of EVERY row of the chunk, K / V of
EVERY row of both layers, and the logits and greedy id of one decode step behind it.
Static-batched steps: 64 sequences at staggered depths 1 .. 23 (far below 128: attn_head_kernel hands wo its operand quantised, gate + up
hands down its), steps of 64, 17, 64, 33, 32, .. rows in rotating order: logits and ids of every row, Batch.check_kv() at the end.
Mixed steps: one decode row and two runs per step (33 rows: body TS 64, three output rows on TS 32), and steps whose every row is an output
row (32 rows; on k31 also 49: the logits launch on TS 64)."""
import functools
import threading
import time

import numpy as np
import pytest

import __graft_entry__ as ge
import bd_gemm_shapes as bs
from test_gpu_batch_decode_depth import Batch, rotated
from test_gpu_gemm3_shapes import _mods, compare_chunk, reference
from test_gpu_mixed_batch import Mixed

pytestmark = pytest.mark.gpu
CASES = list(bs.CASES)
ORACLE_SECONDS = {}


@functools.lru_cache(maxsize=None)
def model(case):
    return bs.case_model(_mods()[0], case)


@functools.lru_cache(maxsize=None)
def chunk_reference(case):
    """The 65-token chunk token by token on one oracle; its prefixes are the references of the shorter chunks"""
    pkg = _mods()[0]
    sizes = sorted({n for f, n in bs.steps_of(case) if f == "chunk"})
    t0 = time.perf_counter()
    ref = reference(model(case), sizes, pkg.javarand.bench_tokens(model(case).cfg.vocab, max(sizes) + 1))
    ORACLE_SECONDS[case] = time.perf_counter() - t0
    return ref


def make_plan(case, n_seqs, flags=0):
    return _mods()[2].HipMasterPlan(model(case), prefill_batch_size=65, n_seqs=n_seqs, flags=flags)


def run_chunks(case, flags=0):
    sizes = [n for f, n in bs.steps_of(case) if f == "chunk"]
    ref = chunk_reference(case)
    plan = make_plan(case, len(sizes), flags)
    try:
        for seq, n in enumerate(sizes):
            compare_chunk("%s chunk %d (step %d)" % (case, n, seq), plan, seq, ref, n, bs.CASES[case]["dim"])
    finally:
        plan.freeTornadoExecutionPlan()


def run_batch(case, flags=0):
    pkg, orc = _mods()[:2]
    m = model(case)
    counts = [n for f, n in bs.steps_of(case) if f == "batch"]
    lens = [1 + (5 * s) % 23 for s in range(64)]
    plan = make_plan(case, 64, flags)
    oracles = [orc.COracle(m) for _ in lens]
    try:
        b = Batch(orc, plan, oracles, m, lens, seed=31)
        for step, n in enumerate(counts):
            b.step(rotated(list(range(n)), step))
        assert [len(o) for o, _ in b.log] == counts and max(max(at) for _, at in b.log) < 128
        b.check_kv()
    finally:
        plan.freeTornadoExecutionPlan()
        [o.close() for o in oracles]


def run_mixed(case, flags=0):
    orc = _mods()[1]
    m = model(case)
    steps = [(f, n) for f, n in bs.steps_of(case) if f.startswith("mixed")]
    n_seqs = 1 + 2 * len(steps)
    plan = make_plan(case, n_seqs, flags)
    oracles = [orc.COracle(m) for _ in range(n_seqs)]
    try:
        b = Mixed(orc, plan, oracles, m, seed=37)
        b.prefill(0, 5)
        fresh = 1
        for form, n in steps:
            single, lengths = bs.mixed_runs(n)
            runs = [(fresh + i, b.tokens(r)) for i, r in enumerate(lengths)]
            fresh += len(lengths)
            if single:
                runs.insert(1 if len(runs) > 1 else 0, (0, b.tokens(1)))          # the decode row between the runs
            assert sum(len(t) for _, t in runs) == n
            b.step(runs, flag_all={s for s, _ in runs} if form == "mixed-all" else ())
    finally:
        plan.freeTornadoExecutionPlan()
        [o.close() for o in oracles]


@pytest.mark.parametrize("case", CASES)
def test_chunks(case):
    run_chunks(case)


@pytest.mark.parametrize("case", CASES)
def test_static_batched_steps(case):
    run_batch(case)


@pytest.mark.parametrize("case", CASES)
def test_mixed_steps(case):
    run_mixed(case)


@pytest.mark.parametrize("case", ["k17", "k31"])
def test_eager_launches(case):
    """FLAG_NO_GRAPH: the static-batched steps enqueued eagerly instead of replayed from their captured graphs; the chunks beside them"""
    hip = _mods()[3]
    run_batch(case, hip.FLAG_NO_GRAPH)
    run_chunks(case, hip.FLAG_NO_GRAPH)


FORMS = [{"GL3_NO_FUSED_QUANT": "1"}, {"GL3_NO_FUSED_BD_ATTN": "1"}]


@pytest.mark.parametrize("env", FORMS, ids=[next(iter(e))[4:].lower() for e in FORMS])
def test_grid_cases_under_a_form(env):
    """k17 (Granite, a ragged tile alone in the partial trip) and k31 (every token count) again, each in its own process (the library reads
    its switches once): GL3_NO_FUSED_QUANT=1 runs the plain SwiGLU form that writes hb as f32 and the separate quantise launch in front of wo
    and down; GL3_NO_FUSED_BD_ATTN=1 the three-kernel attention of the static-batched steps, whose output reaches wo through the quantiser."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-k",
                          "(test_chunks or test_static_batched_steps or test_mixed_steps) and (k17 or k31)", "-p", "no:cacheprovider"],
                         capture_output=True, text=True, timeout=300, env=dict(os.environ, **env), cwd=root)
    tail = out.stdout[-1500:] + out.stderr[-500:]
    assert out.returncode == 0, tail
    assert "6 passed" in out.stdout and "failed" not in out.stdout and "skipped" not in out.stdout, tail


EDGE_EDITS = ["act-blocks", "inner-act-blocks", "w-scales", "w-quants"]


@pytest.mark.parametrize("edits", EDGE_EDITS)
def test_edge_values_at_33_tokens(edits):
    """The edge-value models of tests/edge_models.py (tiny-llama: dim 256, hidden 512) on the 64-slot layout: one chunk of 33 tokens (every
    row compared) and one static-batched step of 33 rows, among them the zero and the flat token: the TS = 64 quantising epilogue of gate + up
    meets zero, f16-subnormal and rounds-to-zero blocks.  (tests/test_gpu_value_edges.py runs chunks of 37 and 20 tokens on act-blocks,
    w-scales and w-quants, comparing x behind the chunk only, and static-batched steps of at most 5 rows.)"""
    import edge_models as em
    pkg, orc, plan_mod, _ = _mods()
    m = em.make_edge_model("tiny-llama", 8, 7, edits)
    toks = em.edge_tokens(pkg, m, 34)
    toks[31], toks[32] = em.FLAT_TOKEN, em.ZERO_TOKEN           # the only row of the third token tile is the zero token
    ref = reference(m, [33], toks)
    assert all(np.all(np.isfinite(ref[k])) for k in ("X", "K", "V")), "the model leaves the finite range"
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=64, n_seqs=34)
    oracles = [orc.COracle(m) for _ in range(33)]
    try:
        compare_chunk("edge %s" % edits, plan, 33, ref, 33, m.cfg.dim)
        b = Batch(orc, plan, oracles, m, [1 + (3 * s) % 11 for s in range(33)], seed=41)
        b.cur[0], b.cur[16], b.cur[31], b.cur[32] = em.ZERO_TOKEN, em.FLAT_TOKEN, em.FLAT_TOKEN, em.ZERO_TOKEN
        b.step(list(range(33)))
        b.check_kv()
    finally:
        plan.freeTornadoExecutionPlan()
        [o.close() for o in oracles]


def test_two_ranks():
    """tp = 2 over the in-process group on k3: dim / 2 = 48 rows = an odd number of strips on wo / down, rank-chunked rows, the f32 hb and
    the separate quantise launch (no quantised hand-over under tensor parallelism).  Chunks of 64, 33 and 17 tokens from position 0 (the
    shorter over the longer one's slots): every rank's K / V slice of every row, and the decode step behind each chunk."""
    _, _, plan_mod, hip = _mods()
    case = bs.TP_CASE
    m, ref = model(case), chunk_reference(case)
    sizes, tp, kvl = (64, 33, 17), 2, model(case).cfg.kv_dim // 2
    grp = plan_mod.make_local_group(tp)
    out, err = [None] * tp, [None] * tp

    def rank_main(r):
        try:
            plan = plan_mod.HipMasterPlan(m, prefill_batch_size=65, tp_rank=r, tp_size=tp, local_group=grp)
            try:
                got = []
                for n in sizes:
                    plan.tornadoVMForwardBatchPrefill(ref["toks"][:n], 0)
                    kv = [[plan.kv(l, p) for p in range(n)] for l in range(bs.LAYERS)]
                    got.append((kv, plan.forward_decode(ref["toks"][n], n)))
                out[r] = got
            finally:
                plan.freeTornadoExecutionPlan()
        except Exception as e:   # noqa: BLE001
            err[r] = e

    th = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(tp)]
    [t.start() for t in th]
    [t.join(timeout=300) for t in th]
    assert all(e is None for e in err), err
    assert not any(t.is_alive() for t in th)
    hip.lib().gl3_local_group_destroy(grp)
    for r in range(tp):
        for (kv, nxt), n in zip(out[r], sizes):
            for l in range(bs.LAYERS):
                for p in range(n):
                    k, v = kv[l][p]
                    assert np.array_equal(k, ref["K"][l][p][r * kvl:(r + 1) * kvl]) and np.array_equal(v, ref["V"][l][p][r * kvl:(r + 1) * kvl]), (r, n, "kv", l, p)
            assert np.array_equal(nxt, ref["behind"][n]), (r, n, "decode behind the chunk")
