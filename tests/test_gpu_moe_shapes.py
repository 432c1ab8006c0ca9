"""Qwen2-MoE at the expert counts, top-k, expert sizes and shared-expert sizes where the kernels branch: the grid of tests/moe_shapes.py through
single-token decode (graph replay and eager launches), batched prefill on both sides of 64 tokens, static-batched decode and a mixed step,
bit for bit (np.array_equal on f32) against one C oracle per sequence.

What a case runs follows from its four numbers (moe_shapes.py restates the rule, tests/test_moe_shapes.py checks it):
    moe_router_token                 n_experts + 1 rows in workgroups of 8: the shared-gate row closes a full workgroup (7, 63), sits alone in one
                                     (8, 64) or leaves padding rows that alias it; the last workgroup's softmax / top-k holds one element per lane
                                     up to 64 experts and strides from 65 on (65: index 64 on the second trip; 130: three trips)
    seq_sum_lds<false>(e, E)         short form below 16 experts, scalar tail for E % 4 != 0
    top-k                            1, all experts (1 of 1, 7 of 7, 64 of 64) and the limit of 64
    matvec_q8t_kernel<.., SEL>       the shared expert as ceil(hidden / moe_hidden) extra slots: smaller than one expert (64 on 128), one whole
                                     slot, 96 96 96 32, 64 64 32, three slots behind 64 selected ones; test_separate_shared_launch_form runs the
                                     decode half under GL3_MOE_MERGE_SHARED=0
    expert K / shared K              1, 2, 3 and 5 Q8_0 blocks: the last 4-block tile group of the down projections is padded (PRO_QUANT matvec,
                                     bdw_gemm_kernel<.., GRP>, the dense down projection at shared sizes 64, 96, 160)
    moe_group_kernel / combine       a wavefront owns up to 9 experts; S = 64 n rows of the XQ2 / XS2 operand; 65 terms per row of the combine

Every case proves from the oracle's routing that it is the case it claims to be (moe_shapes.claims)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import __graft_entry__ as ge
import moe_shapes as ms
from test_gpu_batch_decode_depth import Batch
from test_gpu_mixed_batch import Mixed
from test_gpu_moe_batched import batched_routing, compare_kv, prefill_chunk_and_compare

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = list(ms.GRID)


def _mods():
    from importlib import import_module
    from oracle import oracle_c
    oracle_c.build()
    pkg = ge.load_package()
    return pkg, oracle_c, import_module(ge.PKG_NAME + ".plan"), import_module(ge.PKG_NAME + ".hip")


@functools.lru_cache(maxsize=None)
def model(name):
    return ms.case_model(_mods()[0], name)


def oracle(name):
    return _mods()[1].COracle(model(name))


def frozen(a):
    a = np.array(a, copy=True)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def decode_reference(name):
    """Tokens and, per decode step, the oracle's logits, x after every layer, greedy id and the last layer's routing: once per case, read by
    the graph, eager and loader tests."""
    pkg, orc, _, _ = _mods()
    o = oracle(name)
    toks = ms.decode_tokens(pkg)
    steps = []
    for pos, t in enumerate(toks):
        lg, lx = o.forward(t, pos, layer_x=True)
        sel, w, sw = o.moe_routing()
        steps.append((frozen(lg), [frozen(x) for x in lx], orc.argmax(lg), (sel.tolist(), frozen(w), np.float32(sw))))
    o.close()
    return toks, steps


@functools.lru_cache(maxsize=None)
def long_chunk_reference(name):
    """The 65-token chunk token by token on one oracle: x and the last layer's routing of every row, K / V of both layers.  The oracle stays at
    depth 65 for the batched test of the case to go on with."""
    pkg, _, _, _ = _mods()
    m, o = model(name), oracle(name)
    toks = ms.chunk_tokens(pkg)[1]
    X, routing = [], []
    for b, t in enumerate(toks[:ms.LONG]):
        o.prefill([t], b)
        X.append(frozen(o.x()))
        routing.append(o.moe_routing())
    kv = {(l, p): tuple(frozen(r) for r in o.kv(l, p)) for l in range(m.cfg.n_layers) for p in range(ms.LONG)}
    return dict(toks=toks, X=X, routing=routing, kv=kv, oracle=o)


def compare_routing(routing, sel, w, sw, what):
    """routing: per row the oracle's (ids, probabilities, shared gate); sel / w / sw: the rows read back from the plan"""
    for b, (rsel, rw, rsw) in enumerate(routing):
        assert sel[b].tolist() == list(rsel), (what, "expert ids", b)
        assert np.array_equal(w[b], rw) and sw[b] == rsw, (what, "probabilities / shared gate", b)


# ---- 1. single-token decode
def decode_routing(plan):
    k = plan.cfg.n_experts_used
    w = plan.buffer(7, k + 1)
    return plan.buffer(8, k).astype(np.int32), w[:k], w[k]


def decode_walk(name, plan):
    m = model(name)
    toks, steps = decode_reference(name)
    experts, topk = ms.GRID[name][:2]
    for pos, t in enumerate(toks):
        lg, lx, best, (rsel, rw, rsw) = steps[pos]
        got = plan.forward_decode(t, pos)
        for l in range(m.cfg.n_layers):
            assert np.array_equal(plan.layer_x(l), lx[l]), (name, "x", pos, l)
        assert np.array_equal(got, lg), (name, "logits", pos)
        sel, w, sw = decode_routing(plan)
        assert sel.tolist() == rsel and np.array_equal(w, rw) and sw == rsw, (name, "routing", pos)
        assert plan.forward_decode_argmax(t, pos) == best, (name, "argmax", pos)
        if topk == experts:
            assert sorted(rsel) == list(range(experts)), (name, "top-k = E selects every expert", pos)


def decode_case(name, graph):
    _, _, plan_mod, hip = _mods()
    plan = plan_mod.HipMasterPlan(model(name), flags=hip.FLAG_LAYER_TAPS | (0 if graph else hip.FLAG_NO_GRAPH))
    try:
        decode_walk(name, plan)
    finally:
        plan.freeTornadoExecutionPlan()


@pytest.mark.parametrize("name", CASES)
def test_decode_under_graph_replay(name):
    decode_case(name, graph=True)


@pytest.mark.parametrize("name", CASES)
def test_decode_with_eager_launches(name):
    decode_case(name, graph=False)


# ---- 2. batched prefill, static-batched decode, a mixed step
@pytest.mark.parametrize("name", CASES)
def test_batched_steps(name):
    """Sequence 0: a chunk of 17 tokens (past the 16-token tile of the grouped GEMM, the small-batch operand layout); sequence 1: 65 tokens
    (chunk-major operand for the shared expert, XQ2 / XS2 with 65 topk rows for the routed ones); x and routing of every row and the K / V rows
    of both layers after each.  Then a static-batched decode step over sequences 0, 1, 2 at depths 17, 65, 0 with the routing of every row,
    and a mixed step with a run of 4 rows on sequence 2 and decode rows on 0 and 1."""
    pkg, orc, plan_mod, _ = _mods()
    m = model(name)
    dim = m.cfg.dim
    ref = long_chunk_reference(name)
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=ms.LONG, n_seqs=3)
    try:
        oracles = [oracle(name), ref["oracle"], oracle(name)]
        short = ms.chunk_tokens(pkg)[0]
        short_sel = prefill_chunk_and_compare(plan, oracles[0], short, 0)
        compare_kv(plan, oracles[0], ms.SHORT)
        plan.prefill_seq(1, ref["toks"][:ms.LONG], 0)
        X = plan.buffer(4, ms.LONG * dim).reshape(ms.LONG, dim)
        for b in range(ms.LONG):
            assert np.array_equal(X[b], ref["X"][b]), (name, "x of the long chunk", b)
        long_sel, w, sw = batched_routing(plan, ms.LONG)
        compare_routing(ref["routing"], long_sel, w, sw, (name, "long chunk"))
        for (l, p), (ko, vo) in ref["kv"].items():
            k, v = plan.kv_seq(1, l, p)
            assert np.array_equal(k, ko) and np.array_equal(v, vo), (name, "kv of the long chunk", l, p)
        # the case is the case it claims to be, by the oracle's routing (which the plan's has just been compared with)
        assert ms.claims(name, [r.tolist() for r in short_sel], [list(r[0]) for r in ref["routing"]]) == [], name
        b = Batch(orc, plan, oracles, m, [0, 0, 0], seed=23)      # nothing more to prefill: the chunks above are the prompts
        b.pos = [ms.SHORT, ms.LONG, 0]
        b.cur[1] = int(ref["toks"][ms.LONG])
        b.step([0, 1, 2])
        assert b.log == [([0, 1, 2], [ms.SHORT, ms.LONG, 0])]
        sel, w, sw = batched_routing(plan, 3)
        compare_routing([o.moe_routing() for o in oracles], sel, w, sw, (name, "static-batched step"))
        b.check_kv()
        mixed = Mixed(orc, plan, oracles, m, seed=29)
        mixed.pos = list(b.pos)
        mixed.step([(2, mixed.tokens(4)), (0, [b.cur[0]]), (1, [b.cur[1]])])
        assert mixed.pos == [ms.SHORT + 2, ms.LONG + 2, 5]
        sel, w, sw = batched_routing(plan, 6)                      # rows 0 .. 3: the run on sequence 2 (its last row is the oracle's last step)
        compare_routing([oracles[2].moe_routing()], sel[3:4], w[3:4], sw[3:4], (name, "mixed step, last row of the run"))
        compare_routing([oracles[0].moe_routing(), oracles[1].moe_routing()], sel[4:], w[4:], sw[4:], (name, "mixed step, decode rows"))
    finally:
        plan.freeTornadoExecutionPlan()


# ---- 3. the shared expert's gate / up as a launch of its own
def test_separate_shared_launch_form():
    """GL3_MOE_MERGE_SHARED=0 (read once per process, so a process of its own): launch_matvec_sel without shared slots and the dense gate / up
    launch at the shared sizes 64 .. 1280, over the decode tests of this file."""
    e = dict(os.environ, GL3_MOE_MERGE_SHARED="0")
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q",
                          "-k", "test_decode_under_graph_replay or test_decode_with_eager_launches", "-p", "no:cacheprovider"],
                         capture_output=True, text=True, timeout=600, env=e, cwd=ROOT)
    tail = out.stdout[-1500:] + out.stderr[-500:]
    assert out.returncode == 0, tail
    assert "%d passed" % (2 * len(CASES)) in out.stdout and "failed" not in out.stdout and "skipped" not in out.stdout, tail


# ---- 4. the native loader
def test_native_gguf_loader(tmp_path):
    """e7-k7 (experts of 96, shared expert 320: neither a power of two) written as a "qwen2moe" file and loaded by gl3_load_gguf: the same
    decode steps, bit-identical."""
    _, _, plan_mod, hip = _mods()
    name = "e7-k7"
    path = str(tmp_path / "e7-k7.gguf")
    model(name).write_gguf(path)
    plan = plan_mod.HipMasterPlan.from_gguf(path, flags=hip.FLAG_LAYER_TAPS)
    try:
        c = plan.cfg
        assert (c.arch, c.n_experts, c.n_experts_used, c.moe_hidden, c.hidden, c.dim) == (5, 7, 7, 96, 320, 256)
        decode_walk(name, plan)
    finally:
        plan.freeTornadoExecutionPlan()
