"""The serving surface on row-split ranks: the mixed batched step (gl3_forward_batch), the batched sampler and the token scores with
tp_size > 1.  Ranks are host threads on one GPU (make_local_group); every rank is called with the same arguments and must return the same
outputs.

References: one CPU oracle per sequence slot (orc.COracle), orc.sample, and ref_scores of test_gpu_token_score.py — never a one-rank plan of
the library.  Every comparison is np.array_equal / an exact id: a row-split rank computes whole dot products in the reference's order, and
every rank samples or scores from the same gathered logits with the same coins.  All references are computed on the main thread before
the ranks start.

Two cases run in a fresh process each (this file as a script): four polling ranks late in a long-lived process can end up sharing a
hardware queue (tests/conftest.py), and GL3_PF_TAB_MAXPOS, which makes a 640-position context split a step by depth, is read once per
process."""
import dataclasses
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)                 # script mode; under pytest conftest.py has done it

import __graft_entry__ as ge  # noqa: E402
from test_gpu_mixed_batch import schedule  # noqa: E402
from test_gpu_token_score import FIELDS, ref_scores  # noqa: E402
from test_gpu_tp import kv_slices_equal, model_at, run_ranks  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
UNSUPPORTED = -2                                 # GL3_E_UNSUPPORTED (include/gpullama3_hip.h)


@pytest.fixture(scope="module")
def planmod():
    from importlib import import_module
    ge.load_package()
    return import_module(ge.PKG_NAME + ".plan"), import_module(ge.PKG_NAME + ".hip")


def variant(pkg, cfg, seed, wtype=8, **over):
    return pkg.synth.make_numpy(dataclasses.replace(pkg.synth.CONFIGS[cfg], **over), wtype=wtype, seed=seed)


def meeting(tp):
    """-> meet(): the ranks of an in-process group wait for each other on the host.  The sampler captures its launches into a graph at the first
    step of a shape, and a blocking copy on the null stream from another thread of the process (sample_probs_row) invalidates a capture in
    progress; ranks in one process therefore read the probabilities only once every rank's sampled step has returned, and go on together.
    (One process per GPU, the production layout, has no such neighbour.)"""
    bar = threading.Barrier(tp)
    return lambda: bar.wait(timeout=120)


def oracle_for(orc, m, wtype):
    return orc.COracle(m, vector_bits=256) if wtype != 8 else orc.COracle(m)


class Recorder:
    """What schedule(b) of test_gpu_mixed_batch.py drives, on the oracles alone: step(runs) runs every row on its sequence's oracle and records
    the step's arrays and the oracle's logits / greedy ids of its output rows; the ranks replay the record."""

    def __init__(self, orc, oracles, m, seed):
        self.orc, self.oracles, self.m = orc, oracles, m
        self.rng = np.random.default_rng(seed)
        self.pos = [0] * len(oracles)
        self.next_id = {}
        self.steps, self.kv_keys = [], []

    def tokens(self, n):
        return self.rng.integers(0, self.m.cfg.vocab, n).tolist()

    def prefill(self, seq, n):
        t = self.tokens(n)
        self.oracles[seq].prefill(t, self.pos[seq])
        self.steps.append(("prefill", seq, t, self.pos[seq]))
        self.pos[seq] += n

    def step(self, runs, flag_all=(), explicit=False, no_outputs=False):
        toks, seqs, poss, want = [], [], [], []
        for seq, t in runs:
            toks += list(t); seqs += [seq] * len(t); poss += list(range(self.pos[seq], self.pos[seq] + len(t)))
            want += [0] * len(t) if no_outputs else [1] * len(t) if seq in flag_all else [0] * (len(t) - 1) + [1]
        logits = []
        for row in range(len(toks)):
            ref = self.oracles[seqs[row]].forward(toks[row], poss[row])
            if want[row]:
                logits.append(ref.copy())
                self.next_id[seqs[row]] = self.orc.argmax(ref)
        self.steps.append(("step", toks, seqs, poss, want if (flag_all or explicit or no_outputs) else None, logits))
        for seq, t in runs:
            p0 = self.pos[seq]
            self.kv_keys += [(seq, l, p) for p in sorted({p0, p0 + len(t) - 1}) for l in range(self.m.cfg.n_layers)]
            self.pos[seq] += len(t)

    def kv(self):
        """oracle K / V of the first and last position of every run, every layer (a position is written once: read at the end)"""
        return {key: self.oracles[key[0]].kv(key[1], key[2]) for key in self.kv_keys}


def replay(plan, steps, kv_keys):
    """A rank's side of a record -> ([(logits, ids, attn_rows) per step], {key: its K / V slice})"""
    out = []
    for s in steps:
        if s[0] == "prefill":
            plan.prefill_seq(s[1], s[2], s[3])
            continue
        _, toks, seqs, poss, want, _ = s
        lg, ids = plan.forward_batch(toks, seqs, poss, want)
        out.append((None if lg is None else lg.copy(), ids.copy(), plan.attn_rows()))
    return out, {key: plan.kv_seq(*key) for key in kv_keys}


def assert_replay(orc, rec, out, tp, expect_rows=None):
    """every rank's outputs of every step equal the oracle's and rank 0's; its K / V slices equal the oracle's; attn_rows sums to the step's rows"""
    ref_kv = rec.kv()
    kvl = rec.m.cfg.kv_dim // tp
    steps = [s for s in rec.steps if s[0] == "step"]
    for r, (res, kv) in enumerate(out):
        assert len(res) == len(steps)
        for i, ((lg, ids, rows), (_, toks, _, _, _, ref)) in enumerate(zip(res, steps)):
            assert len(ids) == len(ref) and (lg is None) == (not ref), (r, i)
            for k, want in enumerate(ref):
                assert np.array_equal(lg[k], want), ("logits", "rank", r, "step", i, "output row", k)
                assert int(ids[k]) == orc.argmax(want), ("id", "rank", r, "step", i, "output row", k)
            assert sum(rows) == len(toks), (r, i, rows)
            if expect_rows is not None:
                assert rows == expect_rows[i], (r, i, rows)
            lg0, ids0, rows0 = out[0][0][i]
            assert np.array_equal(ids, ids0) and rows == rows0 and (lg is None or np.array_equal(lg, lg0)), ("ranks differ", r, i)
        for key in ref_kv:
            assert kv_slices_equal(kv[key], ref_kv[key], r, kvl), ("kv", r) + key


# ---- 1. schedule parity
def check_schedule(pkg, orc, planmod, cfg, wtype, over, tp):
    """schedule(b) — two prompt runs; decode rows around a 17-row run (three attention tiles) whose every row is an output row; a continuation
    chunk from position 17, two decode rows and a one-row run with explicit flags — then a step without output rows (a chunk from position 1
    and one from position 5) and, twice, a step of four single wanted rows (the static-batched step's captured graph, then its replay)."""
    plan_mod, _ = planmod
    m = variant(pkg, cfg, seed=61, wtype=wtype, **over)
    rec = Recorder(orc, [oracle_for(orc, m, wtype) for _ in range(4)], m, seed=7)
    schedule(rec)
    rec.step([(3, rec.tokens(6)), (2, rec.tokens(2))], no_outputs=True)
    for _ in range(2):
        rec.step([(s, rec.tokens(1)) for s in (2, 0, 3, 1)])
    assert rec.pos == [13, 24, 9, 9]
    steps = [s for s in rec.steps if s[0] == "step"]
    assert [len(s[5]) for s in steps] == [2, 19, 4, 0, 4, 4]

    def make_plan(r, grp):
        return plan_mod.HipMasterPlan(m, prefill_batch_size=64, n_seqs=4, tp_rank=r, tp_size=tp, local_group=grp)

    out = run_ranks(planmod, tp, make_plan, lambda r, plan: replay(plan, rec.steps, rec.kv_keys))
    assert_replay(orc, rec, out, tp)


SCHEDULE_CASES = [("tiny-llama", 8, {}),                    # head size 32, one kv head per rank
                  ("mid-llama", 8, {}),                     # head size 64, four kv heads per rank
                  ("mid-qwen3", 8, {"ctx": 64}),            # head size 128, q / k norm
                  ("mid-qwen2", 8, {}),                     # kvMul 6, bias, one kv head per rank
                  ("mid-llama", 2, {}),                     # Q4_0: the vector-order layers (pf_layers_vl)
                  ("mid-llama", 1, {})]                     # F16


@pytest.mark.parametrize("cfg,wtype,over", SCHEDULE_CASES, ids=["%s-%d" % (c, w) for c, w, _ in SCHEDULE_CASES])
def test_schedule_parity_tp2(pkg, orc, planmod, cfg, wtype, over):
    check_schedule(pkg, orc, planmod, cfg, wtype, over, 2)


def run_child(*args, env=None):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + [str(a) for a in args], env=dict(os.environ, **(env or {})), cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "child OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_schedule_parity_tp4():
    """mid-llama Q8_0 on four ranks (two kv heads per rank), in a process of its own"""
    run_child("schedule", "mid-llama", 8, 4)


# ---- 2. depth split
def check_depth_split(pkg, orc, planmod):
    """tiny-llama, 640 positions, two ranks: slot 0 is prefilled to position 560, then one step holds its decode row beside a fresh 12-row prompt
    run on slot 1.  Head size 32 keeps a tile's score rows in LDS at any of these depths, so the step is split by GL3_PF_TAB_MAXPOS=511 (the limit
    head size 128 has by itself): the run's tiles on the one-launch table form, the decode row on the long-context trio, on this rank's heads."""
    assert os.environ.get("GL3_PF_TAB_MAXPOS") == "511"
    plan_mod, _ = planmod
    tp = 2
    m = model_at(pkg, "tiny-llama", 640, 8, seed=65)
    rec = Recorder(orc, [orc.COracle(m) for _ in range(2)], m, seed=11)
    rec.prefill(0, 560)
    rec.step([(0, rec.tokens(1)), (1, rec.tokens(12))])
    assert rec.pos == [561, 12]

    def make_plan(r, grp):
        return plan_mod.HipMasterPlan(m, prefill_batch_size=64, n_seqs=2, tp_rank=r, tp_size=tp, local_group=grp)

    out = run_ranks(planmod, tp, make_plan, lambda r, plan: replay(plan, rec.steps, rec.kv_keys))
    assert_replay(orc, rec, out, tp, expect_rows=[[0, 12, 1, 0]])
    for res, _ in out:
        rows = res[0][2]
        assert rows[1] > 0 and rows[2] > 0, rows


def test_depth_split_tp2():
    run_child("depth", env={"GL3_PF_TAB_MAXPOS": "511"})


# ---- 3. sampled steps
SETTINGS = [(0.0, 0.9), (1.0, 0.0), (0.7, 0.95)]            # greedy, categorical, top-p: one row each in every step


def coins_for(rng, n):
    c = rng.random(n).astype(F32)
    return np.minimum(c, np.nextafter(F32(1.0), F32(0.0)))


@pytest.mark.parametrize("cfg", ["tiny-llama", "mid-llama"])
def test_sampled_steps_tp2(pkg, orc, planmod, cfg):
    """forward_decode_batch_sample (three rows) and forward_batch_sample (a 5-row prompt chunk and two decode rows: three output rows) with a
    greedy, a categorical and a top-p row in one step, each step shape twice (capture, then replay of the sampler's graph).  Ids equal
    orc.sample on the oracle's logits, the probabilities of the sampled rows equal the oracle's softmax."""
    plan_mod, _ = planmod
    tp, nseq = 2, 3
    m = variant(pkg, cfg, seed=71)
    V = m.cfg.vocab
    rng = np.random.default_rng(23)
    oracles = [orc.COracle(m) for _ in range(nseq)]
    pre = [rng.integers(0, V, n).tolist() for n in (3, 5, 2)]
    pos = [len(t) for t in pre]
    for o, t in zip(oracles, pre):
        o.prefill(t, 0)
    te, tpp = [s[0] for s in SETTINGS], [s[1] for s in SETTINGS]
    steps = []                                           # (kind, toks, seqs, poss, coins, [(id, probs)] per output row)
    for kind in ("decode", "decode", "mixed", "mixed"):
        runs = [(s, rng.integers(0, V, 5 if (kind == "mixed" and s == 0) else 1).tolist()) for s in range(nseq)]
        toks, seqs, poss, ref = [], [], [], []
        coins = coins_for(rng, nseq)
        for s, t in runs:
            for i, tok in enumerate(t):
                lg = oracles[s].forward(tok, pos[s] + i)
            # the run's last row is its output row
            ref.append(orc.sample(lg, te[s], tpp[s], float(coins[s]), want_probs=True) if te[s] > 0 else (orc.argmax(lg), None))
            toks += t; seqs += [s] * len(t); poss += list(range(pos[s], pos[s] + len(t)))
            pos[s] += len(t)
        steps.append((kind, toks, seqs, poss, coins, ref))

    def make_plan(r, grp):
        return plan_mod.HipMasterPlan(m, prefill_batch_size=16, n_seqs=nseq, tp_rank=r, tp_size=tp, local_group=grp)

    meet = meeting(tp)

    def body(r, plan):
        for s, t in enumerate(pre):
            plan.prefill_seq(s, t, 0)
        res = []
        for kind, toks, seqs, poss, coins, _ in steps:
            if kind == "decode":
                ids = plan.forward_decode_batch_sample(toks, seqs, poss, te, tpp, coins)
            else:
                ids = plan.forward_batch_sample(toks, seqs, poss, te, tpp, coins)
            meet()
            res.append((ids.copy(), [plan.sample_probs_row(k).copy() for k in (1, 2)]))
            meet()
        return res

    out = run_ranks(planmod, tp, make_plan, body)
    for r, res in enumerate(out):
        for i, ((ids, probs), (kind, _, _, _, _, ref)) in enumerate(zip(res, steps)):
            assert [int(x) for x in ids] == [t for t, _ in ref], (r, i, kind)
            for k in (1, 2):
                assert np.array_equal(probs[k - 1], ref[k][1]), ("probs", r, i, k)
            assert np.array_equal(ids, out[0][i][0]), ("ranks differ", r, i)


# ---- 4. the chunked readers without a forward pass
def reader_rows(V, vl, rng):
    """8 rows in the manner of edge_rows (test_gpu_token_score.py) on the edges of both partitions of a row — the rank chunks of vl elements
    and the 4096-element sum chunks: the maximum of row i sits at EDGES[i], row 6 holds equal values, row 7 is flat; the targets visit the
    same indices in another order."""
    edges = [0, vl - 1, vl, 4095, 4096, V - 1]
    lg = rng.standard_normal((8, V)).astype(F32) * F32(3.0)
    for i, e in enumerate(edges):
        lg[i, e] = lg[i].max() + F32(1.0)
    lg[6] = F32(1.5)
    lg[7] *= F32(0.01)
    targets = [vl, 4096, 0, V - 1, vl - 1, 4095, V // 2, int(np.argmax(lg[7]))]
    return lg, targets


@pytest.mark.parametrize("tp", [2, 4])
def test_chunked_readers(pkg, orc, planmod, tp):
    """sample_rows / score_rows on 1, 3 and 8 caller-supplied rows of 8704 logits: on the device they are rank-chunked [tp][rows][4352 | 2176],
    so the 4096-element sum chunks end inside rank chunks and rank boundaries fall inside sum chunks.  No forward pass, no peer."""
    plan_mod, _ = planmod
    V = 8704
    vl = V // tp
    assert vl % 16 == 0 and vl % 4096 and 4096 % vl
    m = variant(pkg, "tiny-llama", seed=5, vocab=V, n_kv_heads=4)
    lg, targets = reader_rows(V, vl, np.random.default_rng(V + tp))
    temps = [1.0, 0.4, 3.0, 0.4, 0.7, 3.0, 1.0, 0.4]
    te = [0.0, 1.0, 0.7, 0.4, 1.3, 0.9, 0.8, 3.0]          # row 0 greedy; rows 2, 4, 6 top-p (row 6: equal values, every rank tied)
    tpp = [0.9, 0.0, 0.95, 1.0, 0.5, 0.0, 0.9, 0.999]
    coins = coins_for(np.random.default_rng(3), 8)
    picks = [[2], [1, 3, 6], list(range(8))]
    want = []
    for rows in picks:
        ids = [orc.sample(lg[i], te[i], tpp[i], float(coins[i])) if te[i] > 0 else orc.argmax(lg[i]) for i in rows]
        sc = ref_scores(lg[rows], [targets[i] for i in rows], [temps[i] for i in rows])
        sc1 = ref_scores(lg[rows], [targets[i] for i in rows], None)
        want.append((ids, sc, sc1))

    def make_plan(r, grp):
        return plan_mod.HipMasterPlan(m, prefill_batch_size=8, tp_rank=r, tp_size=tp, local_group=grp)

    meet = meeting(tp)

    def body(r, plan):
        res = []
        for rows in picks:
            sub, tg = lg[rows], [targets[i] for i in rows]
            ids = plan.sample_rows(sub, [te[i] for i in rows], [tpp[i] for i in rows], coins[rows])
            meet()
            probs = plan.sample_probs_row(len(rows) - 1).copy() if te[rows[-1]] > 0 else None
            meet()
            res.append((ids.copy(), probs, plan.score_rows(sub, tg, [temps[i] for i in rows]).copy(), plan.score_rows(sub, tg).copy()))
        return res

    keep = lg.copy()
    out = run_ranks(planmod, tp, make_plan, body)
    assert np.array_equal(lg, keep)
    for r, res in enumerate(out):
        for rows, (ids, probs, sc, sc1), (ref_ids, ref_sc, ref_sc1) in zip(picks, res, want):
            assert [int(x) for x in ids] == ref_ids, (tp, r, rows, ids.tolist(), ref_ids)
            last = rows[-1]
            assert probs is not None and np.array_equal(probs, orc.sample(lg[last], te[last], tpp[last], float(coins[last]), want_probs=True)[1]), (tp, r, rows)
            for k, f in enumerate(FIELDS):
                assert np.array_equal(sc[f], ref_sc[:, k]), (tp, r, rows, f, sc[f].tolist(), ref_sc[:, k].tolist())
                assert np.array_equal(sc1[f], ref_sc1[:, k]), (tp, r, rows, f, "T = 1")
    # the greedy row's id is the index of its maximum, which sits at index 0; the maxima of rows 1 and 2 sit on either side of the first rank boundary
    assert out[0][2][0][0] == 0 and int(np.argmax(lg[1])) == vl - 1 and int(np.argmax(lg[2])) == vl


# ---- 5. scores through the forward pass
def test_scores_through_the_forward_pass_tp2(pkg, orc, planmod):
    """forward_batch_score on a two-run step — a 9-row prompt chunk with every row wanted beside a 3-row continuation chunk from position 4 —
    with a temperature per output row; the targets are the next tokens."""
    plan_mod, _ = planmod
    tp = 2
    m = variant(pkg, "tiny-llama", seed=91)
    V = m.cfg.vocab
    rng = np.random.default_rng(29)
    oracles = [orc.COracle(m) for _ in range(2)]
    pre = rng.integers(0, V, 4).tolist()
    oracles[1].prefill(pre, 0)
    a, b = rng.integers(0, V, 10).tolist(), rng.integers(0, V, 4).tolist()       # a run's tokens and the token behind it
    toks, seqs, poss = a[:9] + b[:3], [0] * 9 + [1] * 3, list(range(9)) + [4, 5, 6]
    want = [1] * 9 + [0, 0, 1]
    logits = [oracles[0].forward(t, p).copy() for p, t in enumerate(a[:9])]
    for i, t in enumerate(b[:3]):
        last = oracles[1].forward(t, 4 + i)
    logits.append(last.copy())
    targets = a[1:10] + [b[3]]
    temps = [1.0, 0.4, 3.0, 0.7, 1.3, 0.4, 2.0, 0.9, 1.0, 0.6]
    ref = ref_scores(np.array(logits), targets, temps)

    def make_plan(r, grp):
        return plan_mod.HipMasterPlan(m, prefill_batch_size=16, n_seqs=2, tp_rank=r, tp_size=tp, local_group=grp)

    def body(r, plan):
        plan.prefill_seq(1, pre, 0)
        scores, ids = plan.forward_batch_score(toks, seqs, poss, targets, temps, want)
        return scores.copy(), ids.copy()

    out = run_ranks(planmod, tp, make_plan, body)
    for r, (scores, ids) in enumerate(out):
        assert scores.shape == (10,)
        for k, f in enumerate(FIELDS):
            assert np.array_equal(scores[f], ref[:, k]), (r, f, scores[f].tolist(), ref[:, k].tolist())
        assert [int(x) for x in ids] == [orc.argmax(lg) for lg in logits], r
        assert np.array_equal(scores, out[0][0]) and np.array_equal(ids, out[0][1]), ("ranks differ", r)


# ---- 6. the output-row cap
def test_more_than_64_output_rows_are_refused_tp2(pkg, orc, planmod):
    """The gathered logits live in the peer arena, which holds min(max_batch, 64) rows: a 70-row run with every row wanted is refused on both
    ranks with GL3_E_UNSUPPORTED and writes nothing; the same 70 rows with 64 of them wanted equal the oracle."""
    plan_mod, hip = planmod
    tp, n = 2, 70
    m = model_at(pkg, "tiny-llama", 128, 8, seed=77)
    o = orc.COracle(m)
    toks = np.random.default_rng(31).integers(0, m.cfg.vocab, n).tolist()
    ref = [o.forward(t, p).copy() for p, t in enumerate(toks)]
    L = m.cfg.n_layers
    ref_kv = {(l, p): o.kv(l, p) for l in range(L) for p in (0, n - 1)}
    want = [0] * 6 + [1] * 64

    def make_plan(r, grp):
        return plan_mod.HipMasterPlan(m, prefill_batch_size=80, tp_rank=r, tp_size=tp, local_group=grp)

    def body(r, plan):
        before = [plan.kv_seq(0, l, 0) for l in range(L)]
        codes = []
        for call in (lambda: plan.forward_batch(toks, [0] * n, list(range(n)), [1] * n),
                     lambda: plan.forward_batch_sample(toks, [0] * n, list(range(n)), 0.7, 0.9, 0.5, [1] * n),
                     lambda: plan.forward_batch_score(toks, [0] * n, list(range(n)), toks, None, [1] * n)):
            try:
                call()
                codes.append(0)
            except hip.Gl3Error as e:
                codes.append(e.code)
        after = [plan.kv_seq(0, l, 0) for l in range(L)]
        lg, ids = plan.forward_batch(toks, [0] * n, list(range(n)), want)
        return codes, before, after, lg.copy(), ids.copy(), {key: plan.kv_seq(0, *key) for key in ref_kv}

    out = run_ranks(planmod, tp, make_plan, body)
    kvl = m.cfg.kv_dim // tp
    for r, (codes, before, after, lg, ids, kv) in enumerate(out):
        assert codes == [UNSUPPORTED] * 3, (r, codes)
        for (kb, vb), (ka, va) in zip(before, after):
            assert not kb.any() and not vb.any() and not ka.any() and not va.any(), r      # the refused calls wrote no K / V row
        assert lg.shape == (64, m.cfg.vocab)
        for k in range(64):
            assert np.array_equal(lg[k], ref[6 + k]), (r, k)
            assert int(ids[k]) == orc.argmax(ref[6 + k]), (r, k)
        for key in ref_kv:
            assert ref_kv[key][0].any() and kv_slices_equal(kv[key], ref_kv[key], r, kvl), (r,) + key
        assert np.array_equal(lg, out[0][3]) and np.array_equal(ids, out[0][4]), ("ranks differ", r)


if __name__ == "__main__":
    from importlib import import_module
    from oracle import oracle_c
    oracle_c.build()
    _pkg = ge.load_package()
    _planmod = (import_module(ge.PKG_NAME + ".plan"), import_module(ge.PKG_NAME + ".hip"))
    if sys.argv[1] == "schedule":
        check_schedule(_pkg, oracle_c, _planmod, sys.argv[2], int(sys.argv[3]), {}, int(sys.argv[4]))
    elif sys.argv[1] == "depth":
        check_depth_split(_pkg, oracle_c, _planmod)
    else:
        raise SystemExit("usage: test_gpu_tp_batch.py schedule <config> <weight type> <tp> | depth")
    print("child OK")
