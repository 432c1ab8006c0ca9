"""Qwen2-MoE batched prefill and static-batched decode (router with the token as a grid dimension, grouping by expert, the grouped expert
GEMMs over the tile table, shared expert on the dense GEMMs, combine) against the CPU oracle of InferenceCore.forwardJavaQwen2MoE, one
oracle per sequence, stepped token by token.

Everything is np.array_equal on f32: x of every row of a chunk, K / V of every layer at every position, logits and greedy ids of the
decode steps, and the routing of the last layer of every row (expert ids, their probabilities, the shared expert's sigmoid gate) read
back through gl3_get_buffer 9 / 10.

Expert K (= tiles of the routed down projection): tiny-qwen2moe 128 (one tile), mid-qwen2moe 384 (three), a2.7b-moe-layer 1408
(eleven) — all odd counts, which the dense small-batch GEMM had not seen.
"""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as ge
from test_gpu_batch_decode_depth import Batch, model_with_ctx, rotated

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def planmod():
    from importlib import import_module
    ge.load_package()
    return import_module(ge.PKG_NAME + ".plan"), import_module(ge.PKG_NAME + ".hip")


@pytest.fixture(scope="module")
def mid_model(pkg):
    return pkg.synth.make_numpy(pkg.synth.CONFIGS["mid-qwen2moe"], seed=61)


def batched_routing(plan, rows):
    """(expert ids [rows][topk], weights [rows][topk], shared gate [rows]) of the last layer of the last batched step."""
    k = plan.cfg.n_experts_used
    w = plan.buffer(9, rows * (k + 1)).reshape(rows, k + 1)
    sel = plan.buffer(10, rows * k).reshape(rows, k).astype(np.int32)
    return sel, w[:, :k], w[:, k]


def prefill_chunk_and_compare(plan, o, toks, start):
    """One batched chunk on the plan; the oracle token by token.  Compares x and the last layer's routing of every row; returns the ids."""
    n, dim = len(toks), plan.cfg.dim
    plan.tornadoVMForwardBatchPrefill(toks, start)
    X = plan.buffer(4, n * dim).reshape(n, dim)
    sel, w, sw = batched_routing(plan, n)
    for b, t in enumerate(toks):
        o.prefill([t], start + b)                                    # one token, no logits: x stays the residual stream
        assert np.array_equal(X[b], o.x()), ("x", start, b)
        rsel, rw, rsw = o.moe_routing()
        assert sel[b].tolist() == rsel.tolist() and np.array_equal(w[b], rw) and sw[b] == rsw, ("routing", start, b)
    assert np.array_equal(plan.x(), o.x())
    return sel


def compare_kv(plan, o, n_pos):
    for l in range(plan.cfg.n_layers):
        for p in range(n_pos):
            k, v = plan.kv(l, p)
            ko, vo = o.kv(l, p)
            assert np.array_equal(k, ko) and np.array_equal(v, vo), ("kv", l, p)


@pytest.mark.parametrize("n", [3, 17, 96])
def test_prefill_tiny_chunks(pkg, orc, planmod, n):
    """8 experts, top-2, expert K = 128.  3 tokens: 6 assignments on 8 experts, so experts stay empty.  17: past the 16-token tile.  96 tokens
    (max_batch 96): 192 assignments on 8 experts put at least 24 on one, so an expert owns several table entries, and the step is on the
    > 64-token path (chunk-major operand for the shared expert, the XQ2 layout with 96 token slots for the routed ones)."""
    plan_mod, _ = planmod
    m = model_with_ctx(pkg, "tiny-qwen2moe", 160, seed=71)
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=96)
    o = orc.COracle(m)
    toks = pkg.javarand.bench_tokens(m.cfg.vocab, n)
    sel = prefill_chunk_and_compare(plan, o, toks, 0)
    compare_kv(plan, o, n)
    counts = np.bincount(sel.ravel(), minlength=m.cfg.n_experts)
    assert counts.sum() == n * m.cfg.n_experts_used
    if n == 3:
        assert (counts == 0).sum() >= 2, counts
    if n == 96:
        assert counts.max() > 16, counts
    plan.freeTornadoExecutionPlan()


def test_prefill_mid_two_chunks_then_decode(pkg, orc, planmod, mid_model):
    """60 experts, top-4, expert K = 384: 40 tokens (the small-batch operand layout), 80 more at position 40 (> 64 tokens), then 4 single
    decode steps on the caches the chunks left."""
    plan_mod, _ = planmod
    m = mid_model
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=80)
    o = orc.COracle(m)
    toks = pkg.javarand.bench_tokens(m.cfg.vocab, 124)
    prefill_chunk_and_compare(plan, o, toks[:40], 0)
    prefill_chunk_and_compare(plan, o, toks[40:120], 40)
    compare_kv(plan, o, 120)
    for pos in range(120, 124):
        assert np.array_equal(plan.tornadoVMForwardDecode(toks[pos], pos), o.forward(toks[pos], pos)), pos
    plan.freeTornadoExecutionPlan()


def test_prefill_at_the_a2_7b_layer_shapes(pkg, orc, planmod):
    """dim 2048, 60 experts of 1408 (expert K = 1408 = 11 tiles for the routed down projection), shared expert 5632: 24 tokens, then 72."""
    import torch
    plan_mod, _ = planmod
    m = pkg.synth.make_torch(pkg.synth.CONFIGS["a2.7b-moe-layer"], wtype=8, seed=9, device="cuda" if torch.cuda.is_available() else "cpu")
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=72)
    o = orc.COracle(m)
    toks = pkg.javarand.bench_tokens(m.cfg.vocab, 96)
    prefill_chunk_and_compare(plan, o, toks[:24], 0)
    prefill_chunk_and_compare(plan, o, toks[24:], 24)
    compare_kv(plan, o, 96)
    plan.freeTornadoExecutionPlan()


DECODE_LENS = [9, 3, 14, 1, 6]


@pytest.mark.parametrize("graph", [True, False], ids=["graph-replay", "no-graph"])
def test_static_batched_decode(pkg, orc, planmod, mid_model, graph):
    """n_seqs = 5 with different prompt lengths (the 9- and 14-token prompts enter in two chunks of max_batch 8), 6 steps in rotating row
    order: logits, greedy id and the last layer's routing of every row, then the KV rows the steps wrote."""
    plan_mod, hip = planmod
    m = mid_model
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=8, n_seqs=len(DECODE_LENS), flags=0 if graph else hip.FLAG_NO_GRAPH)
    oracles = [orc.COracle(m) for _ in DECODE_LENS]
    b = Batch(orc, plan, oracles, m, DECODE_LENS, seed=31)
    members = list(range(len(DECODE_LENS)))
    picked = set()
    for step in range(6):
        order = rotated(members, step)
        b.step(order)
        sel, w, sw = batched_routing(plan, len(order))
        for row, s in enumerate(order):
            rsel, rw, rsw = oracles[s].moe_routing()
            assert sel[row].tolist() == rsel.tolist() and np.array_equal(w[row], rw) and sw[row] == rsw, ("routing", step, row, s)
            picked.update(sel[row].tolist())
    assert all(b.log[i][0] != b.log[i + 1][0] for i in range(5)) and len({tuple(o) for o, _ in b.log}) >= 5      # the row order moves every step
    assert len(picked) > m.cfg.n_experts_used
    b.check_kv()
    plan.freeTornadoExecutionPlan()


def test_batched_sampler_equals_the_single_sequence_sampler(pkg, planmod, mid_model):
    """A greedy, a categorical and a top-p row in one gl3_forward_decode_batch_sample step: the ids equal gl3_forward_decode_sample on a
    single-sequence plan fed the same tokens (the row's whole history, replayed) and the same coins."""
    plan_mod, _ = planmod
    m = mid_model
    settings = [(0.0, 0.9), (1.0, 0.0), (0.7, 0.95)]
    lens = [4, 2, 6]
    batch = plan_mod.HipMasterPlan(m, prefill_batch_size=8, n_seqs=3)
    single = plan_mod.HipMasterPlan(m)
    rng = np.random.default_rng(5)
    hist = [rng.integers(0, m.cfg.vocab, n + 1).tolist() for n in lens]          # prompt + the first token to decode
    for s in range(3):
        batch.prefill_seq(s, hist[s][:-1], 0)
    jr = pkg.javarand.L32X64MixRandom(77)
    for step in range(3):
        coins = [jr.next_float() if settings[s][0] > 0 else 0.0 for s in range(3)]
        order = [0, 1, 2] if step % 2 == 0 else [2, 0, 1]
        ids = batch.forward_decode_batch_sample([hist[s][-1] for s in order], order, [len(hist[s]) - 1 for s in order],
                                                [settings[s][0] for s in order], [settings[s][1] for s in order], [coins[s] for s in order])
        for row, s in enumerate(order):
            single.reset_kv()
            for i, t in enumerate(hist[s][:-1]):
                single.tornadoVMForwardPrefill(t, i)
            want = single.forward_decode_sample(hist[s][-1], len(hist[s]) - 1, settings[s][0], settings[s][1], coins[s])
            assert int(ids[row]) == want, (step, s, settings[s], coins[s])
        for row, s in enumerate(order):
            hist[s].append(int(ids[row]))
    batch.freeTornadoExecutionPlan()
    single.freeTornadoExecutionPlan()


def test_batched_plan_limits(pkg, planmod):
    plan_mod, hip = planmod
    c = pkg.synth.CONFIGS["tiny-qwen2moe"]

    def desc(**over):
        d = hip.ModelDesc(C.sizeof(hip.ModelDesc), c.arch, c.dim, c.hidden, c.n_layers, c.n_heads, c.n_kv_heads, c.head_size, c.vocab, c.ctx,
                          c.rms_eps, 8, 8, 0, 0, 1, 0, 2, 1.0, 0.0, 1.0, 1.0, c.n_experts, c.n_experts_used, c.moe_hidden)
        for k, v in over.items():
            setattr(d, k, v)
        return d
    h = C.c_void_p()
    L = hip.lib()
    assert L.gl3_create(C.byref(desc()), C.byref(h)) == 0                      # n_seqs = 2, max_batch = 8
    L.gl3_destroy(h)
    for over in (dict(tp_size=2), dict(max_batch=1), dict(weight_type=1), dict(weight_type=2), dict(flags=hip.FLAG_F32_ACTIVATION)):
        assert L.gl3_create(C.byref(desc(**over)), C.byref(h)) == -2, over
    for over in (dict(max_batch=65536), dict(max_batch=40000)):                # gridDim.y of the router; max_batch * topk <= 65536
        assert L.gl3_create(C.byref(desc(**over)), C.byref(h)) == -1, over
