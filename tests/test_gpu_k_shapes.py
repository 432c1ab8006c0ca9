"""Every projection path at the inner dimensions where its kernels change form, and at the largest its plan accepts: the grid of
tests/k_shapes.py through single-token decode, batched prefill on both sides of 64 tokens, static-batched decode and a mixed step, bit for
bit (np.array_equal on f32) against one CPU oracle per sequence in the oracle mode of the weight type.

What a case runs follows from its K (k_shapes.py restates the rule, tests/test_k_shapes.py checks it):
    sum of squares of every RMSNorm      exact_sumsq_lds for 1024 <= K <= 5120, seq_sum_lds on one wavefront otherwise — in matvec_q8t_kernel,
                                         pf_norm_quant_kernel<PQ_NORM | PQ_NORM_F32> (every batched step), rmsnorm_f32_kernel (scalar order; vector
                                         order outside the range, and the K-split types with few row groups), the fused prologue of
                                         matvec_vl_kernel (inside the range) and moe_router_token
    matvec_q8t_kernel prologue           the row stays in registers up to K = 5120 (RMS) / 14336 (plain: wo, down), a loop re-reads it above
    moe_router_token                     the router rows' quads in registers up to dim 2048, the late-load loop above
    LDS                                  pf_norm_quant_kernel asks for more than 64 KB from K = 9344; the largest dim (Q8_0: 12416, the gate/up
                                         launch; scalar order: 23296, rmsnorm_f32_kernel; vector order: 16384; 8 experts: 4160, the router) and
                                         hidden (31872, the down launch) run here, the next legal step is refused by gl3_create
"""
import functools
import threading

import numpy as np
import pytest

import __graft_entry__ as ge
import k_shapes as ks
from test_gpu_batch_decode_depth import Batch
from test_gpu_mixed_batch import Mixed
from test_gpu_moe_batched import batched_routing, prefill_chunk_and_compare
from test_k_shapes import _create

pytestmark = pytest.mark.gpu

STEPS = 3                      # single-token decode steps at positions 0 .. 2
SHORT, LONG = 3, 65            # chunks on the <= 64-token GEMM and on the smallest step of the > 64-token path
ALL = sorted(ks.GRID, key=lambda n: (ks.GRID[n][0], ks.GRID[n][1]))
BATCHED = [n for n in ALL if ks.KINDS[ks.GRID[n][0]]["batched"]]
EAGER = [n for n in ALL if ks.GRID[n][0] in ("q8", "q8h")] + ["f16v256-5120", "f16v512-5120", "q4v256-5120", "f16s-5120", "q4s-5120", "q8f32-5120", "moe-2080"]
TP_CASES = ["q8-5152", "q8-8192"]      # dim % 64 != 0: Wo in the padded row split; replicated Wo


def _mods():
    from importlib import import_module
    from oracle import oracle_c
    oracle_c.build()
    pkg = ge.load_package()
    return pkg, oracle_c, import_module(ge.PKG_NAME + ".plan"), import_module(ge.PKG_NAME + ".hip")


@functools.lru_cache(maxsize=None)
def model(name):
    return ks.case_model(_mods()[0], name)


def oracle(name):
    bits, f32act = ks.KINDS[ks.GRID[name][0]]["oracle"]
    return _mods()[1].COracle(model(name), vector_bits=bits, f32_activation=f32act)


def frozen(a):
    a = np.array(a, copy=True)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def decode_reference(name):
    """Tokens and, per decode step, the oracle's logits, x after every layer and greedy id: once per case, read by the graph, eager and
    tensor-parallel tests."""
    pkg, orc, _, _ = _mods()
    m, o = model(name), oracle(name)
    toks = pkg.javarand.bench_tokens(m.cfg.vocab, STEPS)
    steps = []
    for pos, t in enumerate(toks):
        lg, lx = o.forward(t, pos, layer_x=True)
        steps.append((frozen(lg), [frozen(x) for x in lx], orc.argmax(lg)))
    o.close()
    return toks, steps


@functools.lru_cache(maxsize=None)
def long_chunk_reference(name):
    """The 65-token chunk token by token on one oracle: x of every row, the last layer's routing (MoE), K / V of both layers, and the logits
    of the token behind it.  The oracle stays at depth 65 for the batched test of the case to go on with."""
    pkg, _, _, _ = _mods()
    m, o = model(name), oracle(name)
    toks = pkg.javarand.bench_tokens(m.cfg.vocab, LONG + 1)
    X, routing = [], []
    for b, t in enumerate(toks[:LONG]):
        o.prefill([t], b)
        X.append(frozen(o.x()))
        if m.cfg.n_experts:
            routing.append(o.moe_routing())
    kv = {(l, p): tuple(frozen(r) for r in o.kv(l, p)) for l in range(m.cfg.n_layers) for p in range(LONG)}
    return dict(toks=toks, X=X, routing=routing, kv=kv, next_logits=frozen(o.forward(toks[LONG], LONG)), oracle=o)


def compare_routing(plan, rows, routing):
    sel, w, sw = batched_routing(plan, rows)
    for b, (rsel, rw, rsw) in enumerate(routing):
        assert sel[b].tolist() == rsel.tolist() and np.array_equal(w[b], rw) and sw[b] == rsw, ("routing", b)


# ---- 1. single-token decode
def decode_walk(name, graph):
    _, _, plan_mod, hip = _mods()
    m = model(name)
    toks, steps = decode_reference(name)
    plan = plan_mod.HipMasterPlan(m, flags=ks.case_flags(hip, name) | hip.FLAG_LAYER_TAPS | (0 if graph else hip.FLAG_NO_GRAPH))
    try:
        for pos, t in enumerate(toks):
            lg, lx, best = steps[pos]
            got = plan.forward_decode(t, pos)
            for l in range(m.cfg.n_layers):
                assert np.array_equal(plan.layer_x(l), lx[l]), (name, "x", pos, l)
            assert np.array_equal(got, lg), (name, "logits", pos)
            assert plan.forward_decode_argmax(t, pos) == best, (name, "argmax", pos)
    finally:
        plan.freeTornadoExecutionPlan()


@pytest.mark.parametrize("name", ALL)
def test_decode_under_graph_replay(name):
    decode_walk(name, graph=True)


@pytest.mark.parametrize("name", EAGER)
def test_decode_with_eager_launches(name):
    decode_walk(name, graph=False)


# ---- 2. batched prefill, static-batched decode, a mixed step
@pytest.mark.parametrize("name", BATCHED)
def test_batched_steps(name):
    """Sequence 0: a chunk of 3 tokens (the <= 64-token GEMM and its operand layout); sequence 1: 65 tokens (chunk-major operands); X rows
    and the K / V rows of both layers after each.  Then a static-batched decode step over sequences 0, 1, 2 at depths 3, 65, 0, and a mixed
    step with a run of 4 rows on sequence 2 and decode rows on 0 and 1."""
    pkg, orc, plan_mod, hip = _mods()
    m = model(name)
    dim, moe = m.cfg.dim, bool(m.cfg.n_experts)
    ref = long_chunk_reference(name)
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=LONG, n_seqs=3, flags=ks.case_flags(hip, name))
    try:
        oracles = [oracle(name), ref["oracle"], oracle(name)]
        short = pkg.javarand.bench_tokens(m.cfg.vocab, SHORT + 7)[7:]
        if moe:
            prefill_chunk_and_compare(plan, oracles[0], short, 0)
        else:
            plan.prefill_seq(0, short, 0)
            X = plan.buffer(4, SHORT * dim).reshape(SHORT, dim)
            for b, t in enumerate(short):
                oracles[0].prefill([t], b)
                assert np.array_equal(X[b], oracles[0].x()), (name, "x of the short chunk", b)
        for l in range(m.cfg.n_layers):
            for p in range(SHORT):
                k, v = plan.kv_seq(0, l, p)
                ko, vo = oracles[0].kv(l, p)
                assert np.array_equal(k, ko) and np.array_equal(v, vo), (name, "kv of the short chunk", l, p)
        plan.prefill_seq(1, ref["toks"][:LONG], 0)
        X = plan.buffer(4, LONG * dim).reshape(LONG, dim)
        for b in range(LONG):
            assert np.array_equal(X[b], ref["X"][b]), (name, "x of the long chunk", b)
        if moe:
            compare_routing(plan, LONG, ref["routing"])
        for (l, p), (ko, vo) in ref["kv"].items():
            k, v = plan.kv_seq(1, l, p)
            assert np.array_equal(k, ko) and np.array_equal(v, vo), (name, "kv of the long chunk", l, p)
        b = Batch(orc, plan, oracles, m, [0, 0, 0], seed=23)      # nothing more to prefill: the chunks above are the prompts
        b.pos = [SHORT, LONG, 0]
        b.cur[1] = int(ref["toks"][LONG])
        b.step([0, 1, 2])
        assert b.log == [([0, 1, 2], [SHORT, LONG, 0])]
        b.check_kv()
        mixed = Mixed(orc, plan, oracles, m, seed=29)
        mixed.pos = list(b.pos)
        mixed.step([(2, mixed.tokens(4)), (0, [b.cur[0]]), (1, [b.cur[1]])])
        assert mixed.pos == [SHORT + 2, LONG + 2, 5]
    finally:
        plan.freeTornadoExecutionPlan()


# ---- 3. the limits
@pytest.mark.parametrize("kind,field,value,names_it", ks.REFUSED, ids=["%s-%s-%d" % r[:3] for r in ks.REFUSED])
def test_the_next_step_above_a_limit_is_refused(kind, field, value, names_it):
    """The largest accepted dim / hidden of every limit is a row of the grid above; one legal step further gl3_create answers
    GL3_E_UNSUPPORTED, names the dimension and makes no plan."""
    hip = _mods()[3]
    at_limit = max((n for n in ks.GRID if ks.GRID[n][0] == kind), key=lambda n: ks.GRID[n][1])
    assert ks.GRID[at_limit][1] + ks.KINDS[kind]["step"] == value
    code, msg = _create(hip, at_limit, **{field: value})
    assert code == hip.E_UNSUPPORTED == -2 and names_it in msg, (code, msg)
    assert _create(hip, at_limit)[0] == 0


# ---- 4. tensor parallel
@pytest.mark.parametrize("name", TP_CASES)
def test_two_ranks(name):
    """tp = 2 over the in-process group: 3 decode steps, then the 65-token chunk (pf_norm_quant_kernel reads rank-chunked rows with
    cc = dim / 2, K on the seq_sum_lds side), every rank's K / V slice of the chunk and the decode step behind it."""
    _, _, plan_mod, hip = _mods()
    m = model(name)
    toks, steps = decode_reference(name)
    ref = long_chunk_reference(name)
    tp, kvl = 2, m.cfg.kv_dim // 2
    grp = plan_mod.make_local_group(tp)
    out, err = [None] * tp, [None] * tp

    def rank_main(r):
        try:
            plan = plan_mod.HipMasterPlan(m, prefill_batch_size=LONG, tp_rank=r, tp_size=tp, local_group=grp)
            try:
                dec = [plan.forward_decode(t, p) for p, t in enumerate(toks)]
                plan.tornadoVMForwardBatchPrefill(ref["toks"][:LONG], 0)
                kv = {lp: plan.kv(*lp) for lp in ref["kv"]}
                out[r] = (dec, kv, plan.forward_decode(ref["toks"][LONG], LONG))
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
        dec, kv, nxt = out[r]
        for p in range(STEPS):
            assert np.array_equal(dec[p], steps[p][0]), (name, r, "decode", p)
        for (l, p), (ko, vo) in ref["kv"].items():
            k, v = kv[(l, p)]
            assert np.array_equal(k, ko[r * kvl:(r + 1) * kvl]) and np.array_equal(v, vo[r * kvl:(r + 1) * kvl]), (name, r, "kv", l, p)
        assert np.array_equal(nxt, ref["next_logits"]), (name, r, "decode behind the chunk")
