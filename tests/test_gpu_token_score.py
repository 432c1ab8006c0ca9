"""gl3_score_rows / gl3_forward_batch_score on the GPU: the four fields of every row's gl3_token_score, bit for bit (np.array_equal, no
tolerance) against NumPy's restatement of FloatTensor.softmaxInPlace — v = l / T, max, (float) exp((double) (v - max)), the strictly
sequential f32 sum (oracle_np.seq_sum), e[target] / sum — and prob against the probabilities the C oracle's sampler draws from.

The kernel sums a row 4096 numerators at a time (exact parallel evaluation for chunks of >= 1024 elements, the naive chain below), so
the vocabularies sit on its edges: 1008 (one short chunk, naive), 4096 (one full chunk), 4112 (a 16-element tail continuing an exact
chunk), 9232 (two full chunks and a 1040-element tail on the exact path)."""
import dataclasses

import numpy as np
import pytest

import __graft_entry__ as ge
from oracle import oracle_np

pytestmark = pytest.mark.gpu
F32 = np.float32
FIELDS = ("prob", "logit", "max", "sum")
MAX_BATCH = 8


@pytest.fixture(scope="module")
def planmod():
    from importlib import import_module
    ge.load_package()
    return import_module(ge.PKG_NAME + ".plan"), import_module(ge.PKG_NAME + ".hip")


def ref_scores(logits, targets, temperature):
    """NumPy reference: (prob, logit, max, sum) per row; temperature None = 1 for every row"""
    out = []
    for i, row in enumerate(np.asarray(logits, F32)):
        t = F32(1.0) if temperature is None else F32(temperature[i])
        v = (row / t).astype(F32)
        mx = v.max()
        e = np.exp((v - mx).astype(np.float64)).astype(F32)
        s = F32(oracle_np.seq_sum(e))
        out.append((F32(e[targets[i]] / s), v[targets[i]], mx, s))
    return np.array(out, F32).reshape(len(out), 4)


def assert_scores(got, want, what):
    assert got.shape == (want.shape[0],) and got.dtype.itemsize == 16
    for k, f in enumerate(FIELDS):
        assert np.array_equal(got[f], want[:, k]), (what, f, got[f].tolist(), want[:, k].tolist())


def edge_rows(V, rng):
    """MAX_BATCH rows of logits, their targets and which row holds the spike"""
    last = ((V - 1) // 4096) * 4096                      # first element of the last chunk
    lg = rng.standard_normal((MAX_BATCH, V)).astype(F32) * F32(3.0)
    lg[1, 0] = lg[1].max() + F32(1.0)                    # maximum at index 0
    lg[2, V - 1] = lg[2].max() + F32(1.0)                # ... at V - 1
    lg[3, last] = lg[3].max() + F32(1.0)                 # ... at the first element of the last chunk
    lg[4] = rng.standard_normal(V).astype(F32)
    lg[4, 7] = lg[4].max() + F32(200.0)                  # one logit 200 above the rest
    lg[5] = F32(1.5)                                     # equal logits
    lg[7] *= F32(0.01)
    targets = [0, V - 1, last, last, V // 2, min(4095, V - 2), 4096 if V > 4096 else 1, int(np.argmax(lg[7]))]
    return lg, targets, 4


@pytest.mark.parametrize("V", [1008, 4096, 4112, 9232])
def test_chunk_edges(pkg, orc, planmod, V):
    plan_mod, _ = planmod
    m = pkg.synth.make_numpy(dataclasses.replace(pkg.synth.CONFIGS["tiny-llama"], vocab=V), seed=5)
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=MAX_BATCH)
    lg, targets, spike = edge_rows(V, np.random.default_rng(V))
    keep = lg.copy()
    mixed = [1.0, 0.4, 3.0, 0.4, 0.4, 3.0, 1.0, 0.4]      # the spike row at 0.4: 200 / 0.4 below the maximum
    for temps in (None, mixed):
        got = plan.score_rows(lg, targets, temps)
        assert np.array_equal(lg, keep)
        want = ref_scores(lg, targets, temps)
        assert_scores(got, want, ("V", V, temps))
        assert got["prob"][spike] == 0.0 and got["sum"][spike] >= 1.0 and got["max"][spike] - got["logit"][spike] > 150.0
        assert got["prob"][5] == F32(1.0) / F32(oracle_np.seq_sum(np.ones(V, F32)))       # equal logits: every numerator is 1
        for i in range(MAX_BATCH):
            t = 1.0 if temps is None else temps[i]
            _, probs = orc.sample(lg[i], t, 0, 0.5, want_probs=True)
            assert got["prob"][i] == probs[targets[i]], (V, i, t)
    # one row, each kind in turn: a grid of one workgroup
    for i in (0, 3, spike):
        got = plan.score_rows(lg[i:i + 1], targets[i:i + 1], [mixed[i]])
        assert_scores(got, ref_scores(lg[i:i + 1], targets[i:i + 1], [mixed[i]]), ("V", V, "row", i))
    plan.freeTornadoExecutionPlan()


def both_plans(pkg, plan_mod, cfg, seed, n_seqs, max_batch=32):
    m = pkg.synth.make_numpy(pkg.synth.CONFIGS[cfg], seed=seed)
    return m, plan_mod.HipMasterPlan(m, prefill_batch_size=max_batch, n_seqs=n_seqs), plan_mod.HipMasterPlan(m, prefill_batch_size=max_batch, n_seqs=n_seqs)


def assert_same_kv(m, a, b, seq, positions):
    for p in positions:
        for l in range(m.cfg.n_layers):
            (ka, va), (kb, vb) = a.kv_seq(seq, l, p), b.kv_seq(seq, l, p)
            assert np.array_equal(ka, kb) and np.array_equal(va, vb), ("kv", seq, l, p)


@pytest.mark.parametrize("cfg", ["mid-llama", "tiny-qwen3"])
def test_through_the_forward_pass(pkg, planmod, cfg):
    """Plan `a` scores, plan `b` runs the identical forward_batch and hands its logits to the NumPy reference.  Step 1: a 9-row prompt chunk
    with every row wanted and two decode rows; step 2: the continuation chunk of that prompt (every row wanted) and the two decode rows;
    step 3: no output rows; step 4: three single rows, all wanted.  Targets are the next tokens."""
    plan_mod, _ = planmod
    m, a, b = both_plans(pkg, plan_mod, cfg, seed=91, n_seqs=3)
    rng = np.random.default_rng(29)
    tok = lambda n: rng.integers(0, m.cfg.vocab, n).tolist()
    pre = {1: tok(4), 2: tok(6)}
    for s, t in pre.items():
        a.prefill_seq(s, t, 0); b.prefill_seq(s, t, 0)
    prompt = tok(9 + 5 + 1)                       # chunk, continuation, and the token behind it
    pos = [0, 4, 6]

    def step(runs, want_of, temps):
        """runs: [(seq, tokens, the token that follows the run)]"""
        toks, seqs, poss, want, targets = [], [], [], [], []
        for s, t, nxt in runs:
            toks += t; seqs += [s] * len(t); poss += list(range(pos[s], pos[s] + len(t)))
            w = want_of(s, len(t))
            want += w
            targets += [x for x, f in zip(t[1:] + [nxt], w) if f]
        scores, ids = a.forward_batch_score(toks, seqs, poss, targets, temps(len(targets)) if temps else None, want)
        logits, ref_ids = b.forward_batch(toks, seqs, poss, want)
        assert scores.shape == (len(targets),) and ids.shape == (len(targets),)
        if targets:
            assert_scores(scores, ref_scores(logits, targets, temps(len(targets)) if temps else None), (cfg, runs[0][0], len(toks)))
            assert np.array_equal(ids, ref_ids) and np.array_equal(ids, np.argmax(logits, axis=1))
        assert np.array_equal(a.x(), b.x())
        for s, t, _ in runs:
            assert_same_kv(m, a, b, s, sorted({pos[s], pos[s] + len(t) // 2, pos[s] + len(t) - 1}))
            pos[s] += len(t)
        return ids

    every = lambda s, n: [1] * n
    d1, d2 = tok(1), tok(1)
    ids = step([(0, prompt[:9], prompt[9]), (1, d1, tok(1)[0]), (2, d2, tok(1)[0])], every, None)
    assert ids.size == 11
    mixed = lambda n: [(1.0, 0.4, 3.0)[i % 3] for i in range(n)]
    ids = step([(1, [int(ids[9])], tok(1)[0]), (0, prompt[9:14], prompt[14]), (2, [int(ids[10])], tok(1)[0])], every, mixed)
    assert ids.size == 7
    ids = step([(0, tok(3), 0), (2, tok(2), 0)], lambda s, n: [0] * n, None)              # n_out == 0: a pure prefill
    assert ids.size == 0
    ids = step([(2, tok(1), tok(1)[0]), (0, tok(1), tok(1)[0]), (1, tok(1), tok(1)[0])], every, mixed)      # all single rows, all wanted
    assert ids.size == 3 and pos == [18, 7, 11]
    a.freeTornadoExecutionPlan(); b.freeTornadoExecutionPlan()


def test_refusals(pkg, orc, planmod):
    """A target of -1 or vocab, a temperature of 0, below 0 or NaN and NULL targets are argument errors of both entries, raised before
    anything is enqueued: the KV rows of the plan are untouched and the valid step that follows matches the CPU oracle bit for bit."""
    plan_mod, hip = planmod
    m = pkg.synth.make_numpy(pkg.synth.CONFIGS["tiny-llama"], seed=93)
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=16, n_seqs=2)
    oracles = [orc.COracle(m) for _ in range(2)]
    rng = np.random.default_rng(31)
    V = m.cfg.vocab
    first = rng.integers(0, V, 5).tolist()
    plan.prefill_seq(0, first, 0); oracles[0].prefill(first, 0)
    toks, seqs, poss = rng.integers(0, V, 4).tolist(), [0, 0, 0, 1], [5, 6, 7, 0]

    def kv_rows():
        return [np.concatenate(plan.kv_seq(s, l, p)) for s, p in ((0, 0), (0, 4), (0, 5), (0, 7), (1, 0)) for l in range(m.cfg.n_layers)]
    before = kv_rows()
    lg = rng.standard_normal((2, V)).astype(F32)
    bad = [([-1, 3], None), ([3, V], None), ([3, 4], [1.0, 0.0]), ([3, 4], [-0.5, 1.0]), ([3, 4], [1.0, float("nan")]), (None, None)]
    for targets, temps in bad:
        with pytest.raises(hip.Gl3Error) as ei:
            plan.forward_batch_score(toks, seqs, poss, targets, temps)
        assert ei.value.code == hip.E_ARG, (targets, temps)
        with pytest.raises(hip.Gl3Error) as ei:
            plan.score_rows(lg, targets, temps)
        assert ei.value.code == hip.E_ARG, (targets, temps)
    after = kv_rows()
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    targets, temps = [7, V - 1], [0.4, 3.0]
    scores, ids = plan.forward_batch_score(toks, seqs, poss, targets, temps)
    logits = [oracles[s].forward(t, p) for t, s, p in zip(toks, seqs, poss)]
    out = np.stack([logits[2], logits[3]])
    assert_scores(scores, ref_scores(out, targets, temps), "after the refusals")
    assert ids.tolist() == [orc.argmax(logits[2]), orc.argmax(logits[3])]
    for s, p in ((0, 7), (1, 0)):
        for l in range(m.cfg.n_layers):
            k, v = plan.kv_seq(s, l, p)
            ko, vo = oracles[s].kv(l, p)
            assert np.array_equal(k, ko) and np.array_equal(v, vo)
    plan.freeTornadoExecutionPlan()
    single = plan_mod.HipMasterPlan(m, prefill_batch_size=1)
    with pytest.raises(hip.Gl3Error) as ei:
        single.forward_batch_score([1], [0], [0], [2])
    assert ei.value.code == hip.E_UNSUPPORTED
    with pytest.raises(hip.Gl3Error) as ei:
        single.score_rows(lg[:1], [2])
    assert ei.value.code == hip.E_UNSUPPORTED
    single.freeTornadoExecutionPlan()
