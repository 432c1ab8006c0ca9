"""gl3_verify_rows_dist / gl3_forward_batch_verify_dist and the draft table on the GPU: `accepted` and `token` of every run for exact equality
with the NumPy restatement of the rule (tests/verify_dist_ref.py) — on crafted logits and crafted draft distributions at the edges of the
rule and of the kernel's 4096-element chunks (tests/verify_dist_cases.py; 1008 / 4112 / 9232 as in test_gpu_verify.py), and through the
forward pass of a target and a draft plan against their CPU oracles, the K / V rows of rejected drafts included."""
import dataclasses

import numpy as np
import pytest

import __graft_entry__ as ge
import verify_dist_cases as vc
import verify_dist_ref as vd
import verify_ref as vr

pytestmark = pytest.mark.gpu
F32 = np.float32
TOP = vc.TOP


@pytest.fixture(scope="module")
def planmod():
    from importlib import import_module
    ge.load_package()
    return import_module(ge.PKG_NAME + ".plan"), import_module(ge.PKG_NAME + ".hip")


def as_pairs(res):
    return [(int(a), int(t)) for a, t in zip(res["accepted"], res["token"])]


def slots_of(q_rows, table):
    """q_slots for rows with the distributions q_rows (None: -1); equal distributions share a slot of `table` (a list that grows)"""
    out = []
    for q in q_rows:
        if q is None:
            out.append(-1)
            continue
        hit = [s for s, have in enumerate(table) if np.array_equal(have.view(np.uint32), q.view(np.uint32))]
        if not hit:
            table.append(q)
        out.append(hit[0] if hit else len(table) - 1)
    return out


@pytest.mark.parametrize("V", [1008, 4112, 9232])
def test_verify_rows_dist_on_crafted_logits_and_distributions(pkg, planmod, V):
    plan_mod, _ = planmod
    m = pkg.synth.make_numpy(dataclasses.replace(pkg.synth.CONFIGS["tiny-llama"], vocab=V), seed=5)
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=64)
    T = 0.7
    cases = vc.crafted(V, np.random.default_rng(V), T)
    for case in cases:
        what, lg, tokens, temp, coins, q_rows, accepted, branch = case
        want = vc.check(case)                                           # the case is what its name says
        keep = lg.copy()
        table = []
        q_slots = slots_of(q_rows, table)
        for s, q in enumerate(table):
            plan.draft_probs_put_host(s, q)
            assert np.array_equal(plan.draft_probs(s).view(np.uint32), q.view(np.uint32)), what
        got = plan.verify_rows_dist(lg, tokens, [len(tokens)], [temp], coins, q_slots)
        assert as_pairs(got) == [want], (V, what, as_pairs(got), want)
        assert np.array_equal(lg, keep)
        if what.startswith("one-hot q"):                                # the existing entry on the same coins
            assert as_pairs(plan.verify_rows(lg, tokens, [len(tokens)], [temp], coins)) == [want], (V, what)
            assert as_pairs(plan.verify_rows_dist(lg, tokens, [len(tokens)], [temp], coins, -1)) == [want], (V, what)
    # every run in one call: greedy runs, sampled runs with fixed-token rows, slots shared by two rows, three temperatures
    lg = np.concatenate([c[1] for c in cases])
    tokens = sum((c[2] for c in cases), [])
    run_rows = [len(c[2]) for c in cases]
    temps = [c[3] * (1.0 + 0.5 * (k % 3)) for k, c in enumerate(cases)]
    coins = np.concatenate([c[4] for c in cases])
    table = []
    q_slots = slots_of(sum((c[5] for c in cases), []), table)
    used = [s for s in q_slots if s >= 0]
    assert lg.shape[0] <= 64 and len(table) <= 64 and 0.0 in temps and len({t for t in temps if t > 0}) == 3
    assert len(set(used)) < len(used) and -1 in q_slots                  # a slot read by two rows; fixed-token rows
    for s, q in enumerate(table):
        plan.draft_probs_put_host(s, q)
    want = vd.verify_rows(lg, tokens, run_rows, temps, coins, q_slots, dict(enumerate(table)))
    got = plan.verify_rows_dist(lg, tokens, run_rows, temps, coins, q_slots)
    assert as_pairs(got) == want, (V, "mixed", as_pairs(got), want)
    for s, q in enumerate(table):                                       # the table is read, never written
        assert np.array_equal(plan.draft_probs(s).view(np.uint32), q.view(np.uint32))
    plan.freeTornadoExecutionPlan()


NSEQ, DRAFTS, STEPS = 2, 3, 3
TEMPS = [(0.8, 0.8), (1.1, 0.6)]                                        # (target, draft) temperature of the two sequences


def expected_trajectory(orc, target_model, draft_model, prompts):
    """The three speculative steps of the forward-pass test on the CPU oracles alone -> per step and sequence
    (tokens of the run, position of its first row, q rows, coins [m][2], (accepted, token), whether the draft plan is fed afterwards), and the
    oracles, left where a fourth step continues"""
    to = [orc.COracle(target_model) for _ in range(NSEQ)]
    do = [orc.COracle(draft_model) for _ in range(NSEQ)]
    rng = np.random.default_rng(53)
    pos, last, steps = [], [], []
    for s, p in enumerate(prompts):
        to[s].prefill(p[:-1], 0); do[s].prefill(p[:-1], 0)
        pos.append(len(p) - 1); last.append(p[-1])
    for _ in range(STEPS):
        step = []
        for s in range(NSEQ):
            T, Td = TEMPS[s]
            toks, q_rows, dcoins = [last[s]], [], rng.random(DRAFTS).astype(F32)
            for j in range(DRAFTS):
                q = vr.probs(do[s].forward(toks[j], pos[s] + j), Td)
                toks.append(vr.categorical(q, dcoins[j]))
                q_rows.append(q)
            coins = rng.random((DRAFTS + 1, 2)).astype(F32)
            coins[:, 0] = np.where(rng.random(DRAFTS + 1) < 0.4, F32(TOP), coins[:, 0])      # the largest coin rejects whenever q[d] >= p[d]
            rows = []

            class Lazy:                  # rows behind a rejection saw a token the oracle never forwards: the rule never reads them
                def __getitem__(self, i):
                    while len(rows) <= i:
                        rows.append(to[s].forward(toks[len(rows)], pos[s] + len(rows)).copy())
                    return rows[i]
            a, tok = vd.verify_run(Lazy(), toks, T, coins, q_rows + [None])
            feed = a == DRAFTS
            if feed:
                do[s].forward(toks[DRAFTS], pos[s] + DRAFTS)
            step.append((toks, pos[s], q_rows, dcoins, coins, (a, tok), feed))
            pos[s] += a + 1; last[s] = tok
        steps.append(step)
    return steps, to, do, pos, last


def forward_pass_models(pkg):
    cfg = pkg.synth.CONFIGS["tiny-llama"]
    target = pkg.synth.make_numpy(cfg, seed=61)
    draft = pkg.synth.make_numpy(dataclasses.replace(cfg, n_layers=1), seed=62)
    prompts = [np.random.default_rng(63).integers(0, cfg.vocab, L).tolist() for L in (5, 8)]
    return target, draft, prompts


def test_through_the_forward_pass_of_a_target_and_a_draft_plan(pkg, orc, planmod):
    """Two sequences, each with a draft plan of its own (a plan's single-token step is its sequence 0).  Per step every draft is one
    gl3_forward_decode_sample of the draft plan (its id and its row against the draft oracle) and one gl3_draft_probs_put; the slot equals
    draft.sample_probs() bit for bit; one gl3_forward_batch_verify_dist over both runs equals the restatement on the target oracle's logits.
    The oracles never saw a rejected draft, so a fourth plain step whose logits equal theirs shows that the rejected drafts' K / V rows
    were overwritten before anything read them, on both plans."""
    plan_mod, _ = planmod
    tm, dm, prompts = forward_pass_models(pkg)
    steps, to, do, pos, last = expected_trajectory(orc, tm, dm, prompts)
    results = [st[5] for step in steps for st in step]
    assert any(a == DRAFTS for a, _ in results) and any(0 < a < DRAFTS for a, _ in results) and any(a == 0 for a, _ in results)
    target = plan_mod.HipMasterPlan(tm, prefill_batch_size=16, n_seqs=NSEQ)
    drafts = [plan_mod.HipMasterPlan(dm) for _ in range(NSEQ)]          # max_batch <= 1 is enough for a draft plan
    for s, p in enumerate(prompts):
        target.prefill_seq(s, p[:-1], 0)
        drafts[s].prefill(p[:-1], 0)
    for step in steps:
        toks_all, seqs, poss, coins_all, q_slots = [], [], [], [], []
        for s, (toks, p0, q_rows, dcoins, coins, want, feed) in enumerate(step):
            T, Td = TEMPS[s]
            for j in range(DRAFTS):
                slot = s * DRAFTS + j
                got = drafts[s].forward_decode_sample(toks[j], p0 + j, Td, 0.0, float(dcoins[j]))
                assert got == toks[j + 1], (s, j)
                target.draft_probs_put(slot, drafts[s])
                row = drafts[s].sample_probs()
                assert np.array_equal(row.view(np.uint32), q_rows[j].view(np.uint32)), (s, j)
                assert np.array_equal(target.draft_probs(slot).view(np.uint32), row.view(np.uint32)), (s, j)
                q_slots.append(slot)
            q_slots.append(-7)                                          # the last row of a run never looks at its entry
            toks_all += toks; seqs += [s] * (DRAFTS + 1); poss += list(range(p0, p0 + DRAFTS + 1)); coins_all += list(coins)
        got = as_pairs(target.forward_batch_verify_dist(toks_all, seqs, poss, [t for t, _ in TEMPS], np.asarray(coins_all, F32), q_slots))
        assert got == [st[5] for st in step], (got, [st[5] for st in step])
        for s, (toks, p0, _, _, _, _, feed) in enumerate(step):
            if feed:
                drafts[s].forward_decode(toks[DRAFTS], p0 + DRAFTS)
    for s in range(NSEQ):
        want = to[s].forward(last[s], pos[s])
        got, ids = target.forward_batch([last[s]], [s], [pos[s]])
        assert np.array_equal(got[0], want), s
        assert int(ids[0]) == orc.argmax(want)
        assert np.array_equal(drafts[s].forward_decode(last[s], pos[s]), do[s].forward(last[s], pos[s])), s
    for p in drafts + [target]:
        p.freeTornadoExecutionPlan()


def test_refusals(pkg, orc, planmod):
    """Every refusal comes before anything is enqueued: gl3_get_attn_rows answers as before, the KV rows are untouched and the table keeps
    what it held.  (Plans on different devices need two devices; that refusal is not exercised here.)"""
    plan_mod, hip = planmod
    cfg = pkg.synth.CONFIGS["tiny-llama"]
    m = pkg.synth.make_numpy(cfg, seed=93)
    V = cfg.vocab
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=8, n_seqs=2)
    draft = plan_mod.HipMasterPlan(pkg.synth.make_numpy(dataclasses.replace(cfg, n_layers=1), seed=94))
    other_vocab = plan_mod.HipMasterPlan(pkg.synth.make_numpy(dataclasses.replace(cfg, n_layers=1, vocab=1008), seed=94))
    rng = np.random.default_rng(31)
    first = rng.integers(0, V, 5).tolist()
    plan.prefill_seq(0, first, 0)
    toks, seqs, poss = rng.integers(0, V, 4).tolist(), [0, 0, 0, 1], [5, 6, 7, 0]
    coins = np.full((4, 2), 0.5, F32)
    lg = rng.standard_normal((4, V)).astype(F32)
    q = vr.probs(rng.standard_normal(V).astype(F32), 1.0)

    def kv_rows():
        return [np.concatenate(plan.kv_seq(s, l, p)) for s, p in ((0, 0), (0, 4), (0, 5), (0, 7), (1, 0)) for l in range(cfg.n_layers)]

    def refused(code, call):
        with pytest.raises(hip.Gl3Error) as ei:
            call()
        assert ei.value.code == code, (ei.value, code)
    before, rows_before = kv_rows(), plan.attn_rows()
    # the draft plan has sampled nothing yet / sampled greedily / through top-p
    refused(hip.E_STATE, lambda: plan.draft_probs_put(0, draft))
    assert draft.forward_decode_sample(3, 0, 0.0, 0.0, 0.5) >= 0
    refused(hip.E_STATE, lambda: plan.draft_probs_put(0, draft))
    draft.forward_decode_sample(3, 0, 0.9, 0.9, 0.5)
    refused(hip.E_STATE, lambda: plan.draft_probs_put(0, draft))
    refused(hip.E_STATE, lambda: plan.draft_probs(0))                   # nothing was stored by the refused puts
    draft.forward_decode_sample(3, 0, 0.9, 0.0, 0.5)
    other_vocab.forward_decode_sample(3, 0, 0.9, 0.0, 0.5)
    for call in (lambda: plan.draft_probs_put(0, None), lambda: plan.draft_probs_put(0, plan), lambda: plan.draft_probs_put(-1, draft),
                 lambda: plan.draft_probs_put(8, draft), lambda: plan.draft_probs_put(0, other_vocab),
                 lambda: plan.draft_probs_put_host(0, None), lambda: plan.draft_probs_put_host(-1, q), lambda: plan.draft_probs_put_host(8, q),
                 lambda: plan.draft_probs(-1), lambda: plan.draft_probs(8)):
        refused(hip.E_ARG, call)
    plan.draft_probs_put(2, draft)                                      # the valid put: slot 2 alone is written
    assert np.array_equal(plan.draft_probs(2), draft.sample_probs())
    refused(hip.E_STATE, lambda: plan.draft_probs(1))
    # q_slots: NULL; out of range on a row of a sampled run that has a draft; a slot never written
    for qs in (None, [2, -2, 2, 2], [8, 2, 2, 2]):
        refused(hip.E_ARG, lambda: plan.forward_batch_verify_dist(toks, seqs, poss, [0.7, 0.7], coins, qs))
        refused(hip.E_ARG, lambda: plan.verify_rows_dist(lg, toks, [3, 1], [0.7, 0.7], coins, qs))
    for qs in ([2, 1, 2, 2], [0, 2, 2, 2]):
        refused(hip.E_STATE, lambda: plan.forward_batch_verify_dist(toks, seqs, poss, [0.7, 0.7], coins, qs))
        refused(hip.E_STATE, lambda: plan.verify_rows_dist(lg, toks, [3, 1], [0.7, 0.7], coins, qs))
    refused(hip.E_ARG, lambda: plan.forward_batch_verify_dist(toks, seqs, [5, 6, 8, 0], [0.7, 0.7], coins, 2))      # what the plain entry refuses
    refused(hip.E_ARG, lambda: plan.forward_batch_verify_dist(toks, seqs, poss, [0.7, 0.7], None, 2))
    assert plan.attn_rows() == rows_before
    assert all(np.array_equal(x, y) for x, y in zip(before, kv_rows()))
    # entries nobody looks at: the last row of a run, every row of a greedy run
    want = vd.verify_rows(lg, toks, [3, 1], [0.7, 0.9], coins, [2, -1, 99, -5], {2: plan.draft_probs(2)})
    assert as_pairs(plan.verify_rows_dist(lg, toks, [3, 1], [0.7, 0.9], coins, [2, -1, 99, -5])) == want
    want = vd.verify_rows(lg, toks, [3, 1], [0.0, 0.9], coins, [-1] * 4, {})
    assert as_pairs(plan.verify_rows_dist(lg, toks, [3, 1], [0.0, 0.9], coins, [99, -9, 1, 0])) == want
    for p in (plan, other_vocab):
        p.freeTornadoExecutionPlan()
    single = plan_mod.HipMasterPlan(m, prefill_batch_size=1)
    for call in (lambda: single.draft_probs_put(0, draft), lambda: single.draft_probs_put_host(0, q), lambda: single.draft_probs(0),
                 lambda: single.forward_batch_verify_dist([1], [0], [0], None, None, -1), lambda: single.verify_rows_dist(lg[:1], [2], [1], None, None, -1)):
        refused(hip.E_UNSUPPORTED, call)
    single.freeTornadoExecutionPlan()
    draft.freeTornadoExecutionPlan()


def test_tensor_parallel_plans_are_refused(pkg, orc, planmod):
    """tp_size > 1 (two ranks as threads on one GPU, max_batch > 1): every new entry returns GL3_E_UNSUPPORTED on every rank, as a target and
    (rank 0) as the draft plan of a one-rank target, and enqueues nothing — the static-batched decode step that follows on both ranks
    equals the oracle bit for bit."""
    import threading
    plan_mod, hip = planmod
    tp, nseq = 2, 3
    cfg = pkg.synth.CONFIGS["tiny-llama"]
    m = pkg.synth.make_numpy(cfg, seed=95)
    V = cfg.vocab
    rng = np.random.default_rng(47)
    toks = rng.integers(0, V, nseq).tolist()
    lg = rng.standard_normal((3, V)).astype(F32)
    q = vr.probs(lg[0], 1.0)
    ref = [orc.COracle(m).forward(t, 0) for t in toks]
    draft = plan_mod.HipMasterPlan(pkg.synth.make_numpy(dataclasses.replace(cfg, n_layers=1), seed=96))
    draft.forward_decode_sample(3, 0, 0.9, 0.0, 0.5)
    one_rank = plan_mod.HipMasterPlan(m, prefill_batch_size=8)
    grp = plan_mod.make_local_group(tp)
    out, err = [None] * tp, [None] * tp
    co = np.full((3, 2), 0.5, F32)
    sync = threading.Barrier(tp)

    def rank_main(r):
        try:
            plan = plan_mod.HipMasterPlan(m, prefill_batch_size=8, n_seqs=nseq, tp_rank=r, tp_size=tp, local_group=grp)
            calls = [lambda: plan.draft_probs_put(0, draft), lambda: plan.draft_probs_put_host(0, q), lambda: plan.draft_probs(0),
                     lambda: plan.forward_batch_verify_dist([1, 2, 3], [0, 0, 1], [0, 1, 0], [0.7, 0.0], co, -1),
                     lambda: plan.forward_batch_verify_dist(toks, [0, 1, 2], [0, 0, 0], None, None, -1),
                     lambda: plan.verify_rows_dist(lg, [1, 2, 3], [2, 1], [0.7, 0.0], co, -1)]
            if r == 0:
                calls.append(lambda: one_rank.draft_probs_put(0, plan))
            codes = []
            for call in calls:
                try:
                    call()
                    codes.append(0)
                except hip.Gl3Error as e:
                    codes.append(e.code)
            sync.wait(timeout=120)       # the one-rank plans go before the step: the ranks' polling gathers keep the hardware queues to themselves
            if r == 0:
                draft.freeTornadoExecutionPlan()
                one_rank.freeTornadoExecutionPlan()
            sync.wait(timeout=120)
            out[r] = (codes, plan.forward_decode_batch(toks, [0, 1, 2], [0, 0, 0]))
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
        codes, (logits, ids) = out[r]
        assert codes == [hip.E_UNSUPPORTED] * len(codes) and len(codes) == (7 if r == 0 else 6), (r, codes)
        for s in range(nseq):
            assert np.array_equal(logits[s], ref[s]), (r, s)
            assert int(ids[s]) == orc.argmax(ref[s])
