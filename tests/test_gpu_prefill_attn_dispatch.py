"""A plan without pf_softmax_rows_kernel (context not a multiple of 4, or below 64 positions) has no long-context trio: a one-sequence chunk takes
the one-launch kernels where its rows fit them and the per-row pair everywhere else.  No real model has such a context; two tiny one-layer
models do.

With one layer a row's x behind the layer holds that row's attention output, so every case compares the x rows of every row of every chunk,
the K / V rows at the chunks' edges and the logits of a decode step behind the chunks with np.array_equal against the CPU oracle, and checks
plan.attn_rows(): [attn_head_kernel, one-launch tiled kernels, long-context trio, per-row pair]."""
import numpy as np
import pytest

from test_gpu_mixed_batch import Mixed, planmod  # noqa: F401  (planmod: a fixture)

pytestmark = pytest.mark.gpu


def one_layer_model(pkg, n_heads, n_kv_heads, head_size, ctx, seed):
    cfg = pkg.synth.ModelConfig("attn-dispatch-random", pkg.synth.ARCH_LLAMA, n_heads * head_size, 512, 1, n_heads, n_kv_heads, head_size, 256, ctx,
                                1e-5, 500000.0, False)
    return pkg.synth.make_numpy(cfg, seed=seed)


def run_chunks(pkg, orc, plan_mod, m, batch, chunks, seed):
    """chunks: [(rows, expected attn_rows)] of sequence 0 from position 0, then one decode step (Mixed.step: logits, x, K / V)"""
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=batch, n_seqs=1)
    b = Mixed(orc, plan, [orc.COracle(m)], m, seed=seed)
    o, dim = b.oracles[0], m.cfg.dim
    for n, rows in chunks:
        p0, toks = b.pos[0], b.tokens(n)
        plan.prefill_seq(0, toks, p0)
        assert plan.attn_rows() == rows, (p0, n, plan.attn_rows())
        X = plan.buffer(4, n * dim).reshape(n, dim)
        for i, t in enumerate(toks):              # the oracle row by row: x of every row of the chunk
            o.prefill([t], p0 + i)
            assert np.array_equal(X[i], o.x()), ("x", "pos", p0 + i, "chunk", p0, n)
        assert np.array_equal(plan.x(), o.x()), ("x of the last row", p0, n)
        for p in sorted({p0, p0 + n // 2, p0 + n - 1}):
            k, v = plan.kv_seq(0, 0, p)
            ko, vo = o.kv(0, p)
            assert np.array_equal(k, ko) and np.array_equal(v, vo), ("kv", p)
        b.pos[0] += n
    b.step([(0, b.tokens(1))])
    plan.freeTornadoExecutionPlan()


def test_plan_without_the_rows_softmax(pkg, orc, planmod):
    """Context 150 (not a multiple of 4), head size 128, kvMul 2: the shape has no one-launch kernel (a K tile of 64 x 32 float4 against 8 per
    thread of 128 threads), the plan no trio — chunks of 65 and 40 rows take the per-row pair.  Context 62 (below 64), head size 64, kvMul 4:
    chunks of 37 and 20 rows fit pf_attn_fused3_kernel<64> whole."""
    plan_mod, _ = planmod
    m = one_layer_model(pkg, 4, 2, 128, 150, seed=81)
    run_chunks(pkg, orc, plan_mod, m, 80, [(65, [0, 0, 0, 65]), (40, [0, 0, 0, 40])], seed=21)
    m = one_layer_model(pkg, 8, 2, 64, 62, seed=82)
    run_chunks(pkg, orc, plan_mod, m, 64, [(37, [0, 37, 0, 0]), (20, [0, 20, 0, 0])], seed=22)

