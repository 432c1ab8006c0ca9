"""The batched GEMMs of the f32-activation weight types at every branch of launch_gemm_vl's choice: the grid of tests/vl_gemm_shapes.py, bit
for bit (np.array_equal on f32, no tolerance anywhere) against the CPU oracle in the weight type's mode.

What a grid row reaches follows from the rule (vl_gemm_shapes.py restates it, tests/test_vl_gemm_shapes.py holds it to the library):
    resid           wo / down (48 row tiles, K = 256: one Q4_0 chunk, two Q8_0 chunks): gemm_vlq_kernel at 192 tokens (144 tiles),
                    gemm_vlq_mfma_kernel<EPI_RESID> from 193 (192 tiles, G = 4, P = 2); last token tile of 1, 32 (second half dead), 33 and 64
                    tokens; qkv / gate / up of the same step on gemm_vlq_kernel at K = 3072
    resid-granite   out_scale 0.22 in that residual epilogue
    store           gate / up (48 row tiles, K = 512) on gemm_vlq_mfma_kernel<EPI_STORE> from 193, down (8 row tiles) beside it on gemm_vlq_kernel
    g8              24 row tiles: 448 tokens stay (168 tiles), 449 cross (ntt = 8, G = 8, P = 1), 513 has ntt = 9: one token group with a second tile
    rows            the logits launch over 12304 rows (193 row tiles, the last one of 16 rows): 16 output rows stay on gemm_vlq_kernel, 17 and 32
                    have one token tile whose second half is dead (static-batched decode), 33 and 64 both halves (G = 1, P = 8, 193 % 8 != 0),
                    65 rows of a mixed step G = 2, P = 4, 129 rows ntt = 3 whose fourth tile slot the guard refuses
The F16 species run resid-193, rows-b33 and rows-m65: the same row and token tails on their own kernels and vl_tile_of.

Chunks: every chunk size goes into a fresh sequence from position 0 (one oracle run of the longest chunk, token by token, serves them all):
x of EVERY row of the chunk, K / V of both layers at positions 0, 31, 32, 63, 64, n - 2, n - 1, and the logits of one decode step behind
it.  rows: logits and greedy id of every output row against each sequence's own oracle.  One plan per case and weight type, its steps in
descending and then ascending size (the parametrisation's order), so that a smaller step runs over the stale rows of a larger one.
tests/test_gpu_vl_gemm_forms.py runs rows of this file again under the kernel's A/B switches."""
import functools

import numpy as np
import pytest

import __graft_entry__ as ge
import vl_gemm_shapes as vs
from test_gpu_batch_decode_depth import Batch

pytestmark = pytest.mark.gpu
KV_AT = (0, 31, 32, 63, 64)


def _mods():
    from importlib import import_module
    from oracle import oracle_c
    oracle_c.build()
    pkg = ge.load_package()
    return pkg, oracle_c, import_module(ge.PKG_NAME + ".plan"), import_module(ge.PKG_NAME + ".hip")


def steps_of(case, kind):
    """the case's steps that run this weight type, largest first"""
    s = [r["step"] for r in vs.GRID.values() if r["case"] == case and kind in r["kinds"]]
    return sorted(s, key=vs.ntok_of, reverse=True)


def schedule(mode):
    """(grid row, weight type, leg) in running order: per case and weight type the steps descending, then ascending"""
    out = []
    for case, c in vs.CASES.items():
        if c["mode"] != mode:
            continue
        for kind in c["kinds"] + vs.F16_KINDS:
            down = steps_of(case, kind)
            out += [("%s-%s" % (case, s), kind, leg) for leg, order in (("down", down), ("up", down[::-1])) for s in order]
    return out


@functools.lru_cache(maxsize=None)
def model(case, kind):
    return vs.case_model(_mods()[0], case, kind)


def oracle(case, kind):
    bits, f32act = vs.KINDS[kind]["oracle"]
    return _mods()[1].COracle(model(case, kind), vector_bits=bits, f32_activation=f32act)


def frozen(a):
    a = np.array(a, copy=True)
    a.setflags(write=False)
    return a


# ---- one plan (and its running state) per case and weight type; a new pair releases the one before
_LIVE = {}


def live(case, kind):
    key = (case, kind)
    if key not in _LIVE:
        release()
        _, _, plan_mod, hip = _mods()
        c = vs.CASES[case]
        n_seqs = 2 * len(steps_of(case, kind)) if c["mode"] == "chunk" else 64 + 4
        _LIVE[key] = dict(plan=plan_mod.HipMasterPlan(model(case, kind), prefill_batch_size=c["batch"], n_seqs=n_seqs, flags=vs.kind_flags(hip, kind)),
                          next_seq=0)
    return _LIVE[key]


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
def chunk_reference(case, kind):
    """The longest chunk of the pair token by token on one oracle: x of every row, and at every chunk size n the logits of a decode step of
    token n at position n (taken before that token enters as a prompt token, which rewrites the same K / V row); K / V rows at the end."""
    pkg = _mods()[0]
    m, o = model(case, kind), oracle(case, kind)
    sizes = [vs.ntok_of(s) for s in steps_of(case, kind)]
    top = max(sizes)
    toks = pkg.javarand.bench_tokens(m.cfg.vocab, top + 1)
    X, behind = [], {}
    for b in range(top + 1):
        if b in sizes:
            behind[b] = frozen(o.forward(toks[b], b))
        if b < top:
            o.prefill([toks[b]], b)
            X.append(frozen(o.x()))
    at = sorted({p for n in sizes for p in KV_AT + (n - 2, n - 1)})
    kv = {(l, p): tuple(frozen(r) for r in o.kv(l, p)) for l in range(m.cfg.n_layers) for p in at}
    o.close()
    return dict(toks=toks, X=frozen(np.stack(X)), behind=behind, kv=kv)


CHUNKS = schedule("chunk")


@pytest.mark.parametrize("name,kind,leg", CHUNKS, ids=["%s-%s-%s" % c for c in CHUNKS])
def test_chunk(name, kind, leg):
    orc = _mods()[1]
    case, n = vs.GRID[name]["case"], vs.GRID[name]["step"]
    ref, st, dim = chunk_reference(case, kind), live(case, kind), vs.CASES[case]["dim"]
    plan, seq = st["plan"], st["next_seq"]
    st["next_seq"] += 1
    plan.prefill_seq(seq, ref["toks"][:n], 0)
    X = plan.buffer(4, n * dim).reshape(n, dim)
    bad = [b for b in range(n) if not np.array_equal(X[b], ref["X"][b])]
    assert not bad, (name, kind, "x of rows", bad[:8], "of", len(bad), "columns of the first", np.flatnonzero(X[bad[0]] != ref["X"][bad[0]])[:8].tolist())
    for l in range(vs.LAYERS):
        for p in KV_AT + (n - 2, n - 1):
            k, v = plan.kv_seq(seq, l, p)
            ko, vo = ref["kv"][(l, p)]
            assert np.array_equal(k, ko) and np.array_equal(v, vo), (name, kind, "kv", l, p)
    logits, ids = plan.forward_decode_batch([ref["toks"][n]], [seq], [n])
    assert np.array_equal(logits[0], ref["behind"][n]), (name, kind, "logits of the decode step behind the chunk")
    assert int(ids[0]) == orc.argmax(ref["behind"][n])


# ---- rows
def batch_of(case, kind):
    """The static-batched sequences of the pair: B = the largest step's rows, sequence s prefilled to depth 1 + s % 3, one oracle each"""
    st = live(case, kind)
    if "batch" not in st:
        orc = _mods()[1]
        nseq = max(vs.ntok_of(s) for s in steps_of(case, kind) if s[0] == "b")
        st["batch"] = Batch(orc, st["plan"], [oracle(case, kind) for _ in range(nseq)], model(case, kind), [1 + s % 3 for s in range(nseq)], seed=31)
        st["next_seq"] = 64
    return st["batch"]


@functools.lru_cache(maxsize=None)
def run_reference(case, kind):
    """The longest all-flagged run of the pair on one oracle: the logits of every row"""
    pkg = _mods()[0]
    m, o = model(case, kind), oracle(case, kind)
    top = max(vs.ntok_of(s) for s in steps_of(case, kind) if s[0] == "m")
    toks = pkg.javarand.bench_tokens(m.cfg.vocab, top)
    logits = frozen(np.stack([o.forward(t, p) for p, t in enumerate(toks)]))
    o.close()
    return toks, logits


ROWS = schedule("rows")


@pytest.mark.parametrize("name,kind,leg", ROWS, ids=["%s-%s-%s" % c for c in ROWS])
def test_rows(name, kind, leg):
    orc = _mods()[1]
    case, step = vs.GRID[name]["case"], vs.GRID[name]["step"]
    n = vs.ntok_of(step)
    if step[0] == "b":
        b = batch_of(case, kind)
        b.step(list(range(n)))
        assert b.log[-1][0] == list(range(n)) and max(b.log[-1][1]) < vs.ctx_of(case)
        b.check_kv()
        return
    batch_of(case, kind)                             # the run's sequence lies behind the static-batched ones
    st = live(case, kind)
    plan, seq = st["plan"], st["next_seq"]
    st["next_seq"] += 1
    toks, ref = run_reference(case, kind)
    logits, ids = plan.forward_batch(toks[:n], [seq] * n, list(range(n)), want_logits=[1] * n)
    assert logits.shape == (n, vs.CASES[case]["vocab"])
    bad = [r for r in range(n) if not np.array_equal(logits[r], ref[r])]
    assert not bad, (name, kind, "logits of rows", bad[:8], "of", len(bad), "columns of the first", np.flatnonzero(logits[bad[0]] != ref[bad[0]])[:8].tolist())
    assert ids.tolist() == [orc.argmax(ref[r]) for r in range(n)]
