"""The RMSNorm prologue of matvec_q8t_kernel at the inner dimensions where its paths differ: decode of a one-layer Q8_0 model, bit for bit
against the C oracle, under graph replay and with eager launches.
    1024   the lower end of exact_seqsum_lds
    1056   not a multiple of 128: the last tile group of xq / xs has zero-padded blocks, written ahead of the sum
    5120   the upper end (five segments per thread)
    5152   above it: seq_sum_lds on one wavefront and the re-read of the row, which stay as they were
Every decode step runs the prologue in front of EPI_STORE (qkv, logits) and EPI_SWIGLU (gate/up); the producers start on the count of the
four aux wavefronts' arrivals.  hidden = 2 * dim; 4 heads of dim / 4 where attn_head_kernel takes the head size (256), else the heads of
tests/k_shapes.py (head_size * n_heads need not be dim)."""
import functools

import numpy as np
import pytest

import __graft_entry__ as ge
import k_shapes as ks

pytestmark = pytest.mark.gpu

DIMS = (1024, 1056, 5120, 5152)
STEPS = 2
MAX_HEAD = 256


def _mods():
    from importlib import import_module
    from oracle import oracle_c
    oracle_c.build()
    pkg = ge.load_package()
    return pkg, oracle_c, import_module(ge.PKG_NAME + ".plan"), import_module(ge.PKG_NAME + ".hip")


@functools.lru_cache(maxsize=None)
def model(dim):
    synth = _mods()[0].synth
    heads, kv_heads, hs = (4, 4, dim // 4) if dim % 4 == 0 and dim // 4 <= MAX_HEAD else (ks.HEADS, ks.KV_HEADS, ks.HEAD_SIZE)
    cfg = synth.ModelConfig("prologue-%d" % dim, synth.ARCH_LLAMA, dim, 2 * dim, 1, heads, kv_heads, hs, ks.VOCAB, ks.CTX, 1e-5, 500000.0, False)
    return synth.make_numpy(cfg, wtype=8, seed=43)


@functools.lru_cache(maxsize=None)
def reference(dim):
    """tokens and the oracle's (logits, x after the layer) per step: computed once, read by both modes"""
    pkg, orc, _, _ = _mods()
    m = model(dim)
    o = orc.COracle(m)
    toks = pkg.javarand.bench_tokens(m.cfg.vocab, STEPS)
    steps = []
    for pos, t in enumerate(toks):
        lg, lx = o.forward(t, pos, layer_x=True)
        lg, lx = np.array(lg, copy=True), [np.array(x, copy=True) for x in lx]
        for a in [lg] + lx:
            a.setflags(write=False)
        steps.append((lg, lx))
    o.close()
    return toks, steps


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("dim", DIMS)
def test_decode_matches_the_oracle(dim, graph):
    _, _, plan_mod, hip = _mods()
    assert ks.sumsq_form(dim) == ("exact" if dim <= 5120 else "seq")
    m = model(dim)
    toks, steps = reference(dim)
    plan = plan_mod.HipMasterPlan(m, flags=hip.FLAG_LAYER_TAPS | (0 if graph else hip.FLAG_NO_GRAPH))
    try:
        for pos, t in enumerate(toks):
            lg, lx = steps[pos]
            got = plan.forward_decode(t, pos)
            assert np.array_equal(plan.layer_x(0), lx[0]), (dim, "x", pos)
            assert np.array_equal(got, lg), (dim, "logits", pos)
    finally:
        plan.freeTornadoExecutionPlan()
