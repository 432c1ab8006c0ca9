"""The decode matvecs of the f32-activation weight types at every form of launch_matvec's choice: the grid of tests/matvec_shapes.py, bit for
bit (np.array_equal on f32, no tolerance anywhere: DESIGN §2) against the CPU oracle in the weight kind's mode.

What a case reaches follows from the rule (matvec_shapes.py restates it, tests/test_matvec_shapes.py holds it to the library and shows the
partition of every case): matvec_vlq_kernel at 4, 8 and 16 wavefronts on both sides of 256 and 512 row groups, promoted and halved, with
idle wavefronts, a short last wavefront, two rounds at both MAXW and a ragged last round, in the residual, store and SwiGLU epilogues;
matvec_vl_kernel with and without the RMSNorm prologue for F16 at both species and for the K-split types; matvec_rl_kernel in the scalar order.

Per case and kind: three decode steps from position 0 — x after the layer, the logits, the K / V rows of every position so far and the
device argmax against COracle.  Every case under graph replay; the cases that own the ragged and multi-round partitions once more with eager
launches.  B and D also carry the w-scales / w-quants (Q4_0) and f16-values (F16) edits of tests/edge_models.py."""
import functools
import time

import numpy as np
import pytest

import __graft_entry__ as ge
import edge_models as em
import matvec_shapes as ms

pytestmark = pytest.mark.gpu
STEPS = 3
EDGE = [(c, "q4v256", ("w-scales", "w-quants")) for c in ms.EDGE] + [(c, "f16v256", ("f16-values",)) for c in ms.EDGE]


def _mods():
    from importlib import import_module
    from oracle import oracle_c
    oracle_c.build()
    pkg = ge.load_package()
    return pkg, oracle_c, import_module(ge.PKG_NAME + ".plan"), import_module(ge.PKG_NAME + ".hip")


def frozen(a):
    a = np.array(a, copy=True)
    a.setflags(write=False)
    return a


def walk_oracle(m, kind, toks):
    """the oracle's logits, x after every layer, greedy id and K / V rows of STEPS decode steps, and the seconds they took"""
    orc = _mods()[1]
    bits, f32act = ms.KINDS[kind]["oracle"]
    o = orc.COracle(m, vector_bits=bits, f32_activation=f32act)
    t0 = time.perf_counter()
    steps = []
    for pos, t in enumerate(toks):
        lg, lx = o.forward(t, pos, layer_x=True)
        steps.append((frozen(lg), [frozen(x) for x in lx], orc.argmax(lg)))
    secs = time.perf_counter() - t0
    kv = {(l, p): tuple(frozen(r) for r in o.kv(l, p)) for l in range(m.cfg.n_layers) for p in range(len(toks))}
    o.close()
    assert all(np.all(np.isfinite(s[0])) for s in steps), "the test MODEL leaves the finite range"
    return steps, kv, secs


@functools.lru_cache(maxsize=None)
def reference(case, kind):
    """The model and the oracle's walk: once per case and kind, shared by the graph and the eager test"""
    pkg = _mods()[0]
    m = ms.case_model(pkg, case, kind)
    toks = pkg.javarand.bench_tokens(m.cfg.vocab, STEPS)
    return (m, toks) + walk_oracle(m, kind, toks)


def decode_walk(m, kind, toks, steps, kv, graph, what):
    _, _, plan_mod, hip = _mods()
    plan = plan_mod.HipMasterPlan(m, flags=ms.kind_flags(hip, kind) | hip.FLAG_LAYER_TAPS | (0 if graph else hip.FLAG_NO_GRAPH))
    try:
        for pos, t in enumerate(toks):
            lg, lx, best = steps[pos]
            got = plan.forward_decode(t, pos)
            for l in range(m.cfg.n_layers):
                x = plan.layer_x(l)
                assert np.array_equal(x, lx[l]), (what, "x", pos, l, "rows", np.flatnonzero(x != lx[l])[:8].tolist(), "of", int(np.sum(x != lx[l])))
            assert np.array_equal(got, lg), (what, "logits", pos, "rows", np.flatnonzero(got != lg)[:8].tolist(), "of", int(np.sum(got != lg)))
            for l in range(m.cfg.n_layers):
                for p in range(pos + 1):
                    k, v = plan.kv(l, p)
                    assert np.array_equal(k, kv[(l, p)][0]) and np.array_equal(v, kv[(l, p)][1]), (what, "kv", pos, l, p)
            assert plan.forward_decode_argmax(t, pos) == best, (what, "argmax", pos)
    finally:
        plan.freeTornadoExecutionPlan()


@pytest.mark.parametrize("case,kind", ms.GRID, ids=["%s-%s" % g for g in ms.GRID])
def test_decode_under_graph_replay(case, kind):
    m, toks, steps, kv, secs = reference(case, kind)
    print("oracle seconds of %s-%s: %.2f" % (case, kind, secs))
    decode_walk(m, kind, toks, steps, kv, True, (case, kind))


EAGER = [g for g in ms.GRID if g[0] in ms.EAGER]


@pytest.mark.parametrize("case,kind", EAGER, ids=["%s-%s" % g for g in EAGER])
def test_decode_with_eager_launches(case, kind):
    m, toks, steps, kv, _ = reference(case, kind)
    decode_walk(m, kind, toks, steps, kv, False, (case, kind))


@pytest.mark.parametrize("case,kind,edits", EDGE, ids=["%s-%s" % e[:2] for e in EDGE])
def test_edge_values(case, kind, edits):
    """Zero, subnormal, smallest-normal and 2^15 block scales, nibbles all 0 / all 15 (Q4_0); lane groups of subnormals, signed zeros and
    the largest f16 (F16) in the first and last rows and K blocks of every matrix, at the shapes of B (promoted down, fused gate/up and
    logits) and D (16 wavefronts, a short last one).  F16 runs the case at the Q4_0 kind's dimensions."""
    pkg = _mods()[0]
    d = ms.dims(case, "q4v256")
    m = em.make_edge_model("tiny-llama", ms.KINDS[kind]["wtype"], 7, edits, dim=d["dim"], hidden=d["hidden"], n_layers=1, n_heads=d["heads"],
                           n_kv_heads=d["kv_heads"], head_size=ms.HEAD_SIZE, vocab=d["vocab"], ctx=ms.CTX)
    assert m.edits == edits
    toks = em.edge_tokens(pkg, m, STEPS)
    steps, kv, _ = walk_oracle(m, kind, toks)
    decode_walk(m, kind, toks, steps, kv, True, (case, kind, edits))
