"""The Q8_0 GEMMs of a step of more than 64 rows at every branch of g3_plan's choice and at the edges the kernels are built around: the grid
of tests/gemm3_shapes.py, bit for bit (np.array_equal on f32, no tolerance anywhere) against the CPU oracle.

What a grid row reaches follows from the rule (gemm3_shapes.py restates it, tests/test_gemm3_shapes.py holds it to the library):
    tails           64 x 128 (qkv, wo, down) and the 128 x 128 SwiGLU tiling with a last token tile of 65, 96, 97, 128 tokens alone and of 1, 32,
                    33, 64, 65, 96, 97, 128 behind a full one; K of 5, 8 and 9 blocks, cut last row tiles
    k1 .. k4        one to six K stages at KB 4 and KB 2, a last stage of 1, 2, 3 real blocks, fewer stages than the ring of three
    tall5 / 6 / 7   pf_gemm3t_kernel by default at 385 .. 512 tokens with NFR 5 (2 live fragments in the last row tile), 6 (3), 7 (whole
                    tiles), hb handed to the down projection quantised; tall-end: hidden 14368 is back on 128 x 128
    r96             wo / down on 96 x 128 tiles by default (Granite's out_scale), every token tail; r96-below: dim 3072 stays on 64 x 128
    s96 / s128      the logits launch of a mixed step on 96 x 128 (65 .. 256 flagged rows of vocab 12384; 257: 64 x 128) and on 128 x 128
                    (129 and 161 flagged rows of vocab 32672; 128: 64 x 128); 64 flagged rows of a 65-row and of a 257-row step leave for
                    bdw_gemm_kernel
    edge-tall / edge-r96   the edge-value models of tests/edge_models.py through the default tall kernel and the default 96 x 128 tile
Chunks: every chunk size goes into a fresh sequence from position 0, the longest first, so that a shorter step runs over the stale token
slots of a longer one (one oracle run of the longest chunk, token by token, serves them all): x of EVERY row of the chunk, K / V of EVERY
row of both layers, and the logits of one decode step behind it.  rows: logits and greedy id of every flagged row of the mixed step.
tests/test_gpu_gemm_forms.py runs rows of this file again under the tilings' switches."""
import functools

import numpy as np
import pytest

import __graft_entry__ as ge
import gemm3_shapes as gs

pytestmark = pytest.mark.gpu


def _mods():
    from importlib import import_module
    from oracle import oracle_c
    oracle_c.build()
    pkg = ge.load_package()
    return pkg, oracle_c, import_module(ge.PKG_NAME + ".plan"), import_module(ge.PKG_NAME + ".hip")


def steps_of(case):
    """the case's steps, most rows first"""
    return sorted((r["step"] for r in gs.GRID.values() if r["case"] == case), key=gs.ntok_of, reverse=True)


def schedule(mode):
    return ["%s-%s" % (case, s) for case, c in gs.CASES.items() if c["mode"] == mode for s in steps_of(case)]


@functools.lru_cache(maxsize=None)
def model(case):
    return gs.case_model(_mods()[0], case)


def frozen(a):
    a = np.array(a, copy=True)
    a.setflags(write=False)
    return a


# ---- one plan (and its running state) per case; a new case releases the one before
_LIVE = {}


def live(case):
    if case not in _LIVE:
        release()
        plan_mod = _mods()[2]
        _LIVE[case] = dict(plan=plan_mod.HipMasterPlan(model(case), prefill_batch_size=gs.CASES[case]["batch"], n_seqs=len(steps_of(case))), next_seq=0)
    return _LIVE[case]


def release():
    for st in _LIVE.values():
        st["plan"].freeTornadoExecutionPlan()
    _LIVE.clear()


@pytest.fixture(scope="module", autouse=True)
def _plans():
    yield
    release()


# ---- chunks
@functools.lru_cache(maxsize=None)
def chunk_reference(case):
    """The longest chunk of the case token by token on one oracle: x of every row, and at every chunk size n the logits of a decode step of
    token n at position n (taken before that token enters as a prompt token, which rewrites the same K / V row); K / V of every row at the end."""
    pkg = _mods()[0]
    sizes = [gs.ntok_of(s)[0] for s in steps_of(case)]
    return reference(model(case), sizes, pkg.javarand.bench_tokens(model(case).cfg.vocab, max(sizes) + 1))


def reference(m, sizes, toks):
    o = _mods()[1].COracle(m)
    top = max(sizes)
    X, behind = [], {}
    for b in range(top + 1):
        if b in sizes:
            behind[b] = frozen(o.forward(toks[b], b))
        if b < top:
            o.prefill([toks[b]], b)
            X.append(frozen(o.x()))
    K, V = [], []
    for l in range(m.cfg.n_layers):
        rows = [o.kv(l, p) for p in range(top)]
        K.append(np.stack([r[0] for r in rows]))
        V.append(np.stack([r[1] for r in rows]))
    o.close()
    return dict(toks=toks, X=frozen(np.stack(X)), behind=behind, K=frozen(np.stack(K)), V=frozen(np.stack(V)))


CHUNKS = schedule("chunk")


@pytest.mark.parametrize("name", CHUNKS)
def test_chunk(name):
    case, n = gs.GRID[name]["case"], gs.GRID[name]["step"]
    st = live(case)
    st["next_seq"] += 1
    compare_chunk(name, st["plan"], st["next_seq"] - 1, chunk_reference(case), n, gs.CASES[case]["dim"])


def compare_chunk(name, plan, seq, ref, n, dim):
    """The chunk of n tokens from position 0 into sequence seq: x of every row, K / V of every row of both layers, the decode step behind"""
    orc = _mods()[1]
    plan.prefill_seq(seq, ref["toks"][:n], 0)
    X = plan.buffer(4, n * dim).reshape(n, dim)
    bad = [b for b in range(n) if not np.array_equal(X[b], ref["X"][b])]
    assert not bad, (name, "x of rows", bad[:8], "of", len(bad), "columns of the first", np.flatnonzero(X[bad[0]] != ref["X"][bad[0]])[:8].tolist())
    for l in range(gs.LAYERS):
        kv = [plan.kv_seq(seq, l, p) for p in range(n)]
        bad = [p for p in range(n) if not (np.array_equal(kv[p][0], ref["K"][l][p]) and np.array_equal(kv[p][1], ref["V"][l][p]))]
        assert not bad, (name, "K / V of layer", l, "rows", bad[:8], "of", len(bad))
    logits, ids = plan.forward_decode_batch([ref["toks"][n]], [seq], [n])
    assert np.array_equal(logits[0], ref["behind"][n]), (name, "logits of the decode step behind the chunk")
    assert int(ids[0]) == orc.argmax(ref["behind"][n])


# ---- edge values through the default tall kernel and the default 96 x 128 tile
@pytest.mark.parametrize("case", list(gs.EDGE_CASES))
def test_edge_values_chunk(case):
    """The "all" model of tests/edge_models.py at a shape of gemm3_shapes.EDGE_CASES, one chunk of 385 tokens (the zero token alone in the
    last token tile): the QOUT epilogue of pf_gemm3t_kernel quantises hb blocks that are zero, f16-subnormal in scale, rounded to a zero
    scale and ordinary; 96 x 128 wo / down read zero and subnormal operand blocks and weight scales of 0, 2^-24 and 2^15.  Compared as every
    chunk of this file: every row."""
    pkg, _, plan_mod, _ = _mods()
    release()
    c = gs.EDGE_CASES[case]
    m = gs.edge_model(case)
    ref = reference(m, [c["step"]], gs.edge_tokens(pkg, m, c["step"]))
    assert all(np.all(np.isfinite(ref[k])) for k in ("X", "K", "V")) and np.all(np.isfinite(ref["behind"][c["step"]])), "the model leaves the finite range"
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=c["step"], n_seqs=1)
    try:
        compare_chunk(case, plan, 0, ref, c["step"], c["dim"])
    finally:
        plan.freeTornadoExecutionPlan()


# ---- rows
@functools.lru_cache(maxsize=None)
def run_reference(case):
    """The longest run of the case on one oracle: the logits of every row"""
    pkg, orc = _mods()[:2]
    m, o = model(case), orc.COracle(model(case))
    top = max(gs.ntok_of(s)[0] for s in steps_of(case))
    toks = pkg.javarand.bench_tokens(m.cfg.vocab, top)
    logits = frozen(np.stack([o.forward(t, p) for p, t in enumerate(toks)]))
    o.close()
    return toks, logits


ROWS = schedule("rows")


@pytest.mark.parametrize("name", ROWS)
def test_rows(name):
    orc = _mods()[1]
    case = gs.GRID[name]["case"]
    n, f = gs.ntok_of(gs.GRID[name]["step"])
    st = live(case)
    plan, seq = st["plan"], st["next_seq"]
    st["next_seq"] += 1
    toks, ref = run_reference(case)
    logits, ids = plan.forward_batch(toks[:n], [seq] * n, list(range(n)), want_logits=[0] * (n - f) + [1] * f)
    assert logits.shape == (f, gs.CASES[case]["vocab"])
    want = ref[n - f:n]
    bad = [r for r in range(f) if not np.array_equal(logits[r], want[r])]
    assert not bad, (name, "logits of flagged rows", bad[:8], "of", len(bad), "columns of the first", np.flatnonzero(logits[bad[0]] != want[bad[0]])[:8].tolist())
    assert ids.tolist() == [orc.argmax(want[r]) for r in range(f)]
    served = plan.attn_rows()
    assert sum(served) == n and served[0] == 0, served      # a run of several rows never takes attn_head_kernel
