"""gl3_verify_rows / gl3_forward_batch_verify on the GPU: `accepted` and `token` of every run for exact equality with the NumPy restatement
of the rule (tests/verify_ref.py) — on crafted logits at the edges of the kernel's 4096-element chunks (1008: one short chunk on the naive
chain; 4112: a 16-element tail continuing an exact chunk; 9232: two full chunks and a 1040-element tail — gl3_create takes vocabularies
that are multiples of 16 only) and through the forward pass against the CPU oracle, the KV rows of rejected drafts included."""
import ctypes
import dataclasses

import numpy as np
import pytest

import __graft_entry__ as ge
import verify_ref as vr

pytestmark = pytest.mark.gpu
F32 = np.float32
TOP = float(F32(1.0) - F32(2.0) ** -24)                   # the largest coin rng.nextFloat(1f) can give


@pytest.fixture(scope="module")
def planmod():
    from importlib import import_module
    ge.load_package()
    return import_module(ge.PKG_NAME + ".plan"), import_module(ge.PKG_NAME + ".hip")


def as_pairs(res):
    return [(int(a), int(t)) for a, t in zip(res["accepted"], res["token"])]


def crafted(V, rng, T):
    """[(what, logits [m][V], tokens [m], temperature, coins [m][2], the `accepted` the case is built to give)]"""
    cases = []

    def rows(m):
        return (rng.standard_normal((m, V)) * 3).astype(F32)

    def add(what, lg, tokens, temp, coins, accepted):
        cases.append((what, lg.copy(), [int(t) for t in tokens], temp, np.asarray(coins, F32).reshape(len(tokens), 2), accepted))

    lg = rows(4)
    best = [int(np.argmax(r)) for r in lg]
    worst = [int(np.argmin(r)) for r in lg]
    add("all drafts accepted", lg, [3] + best[:3], T, [(0, .9), (0, .9), (0, .9), (.9, .37)], 3)
    add("rejection at row 0", lg, [3, worst[0], best[1], best[2]], T, [(.5, .61), (0, .9), (0, .9), (.9, .37)], 0)
    add("rejection mid-run", lg, [3, best[0], worst[1], best[2]], T, [(0, .9), (.5, .23), (0, .9), (.9, .37)], 1)
    add("greedy, all accepted", lg, [3] + best[:3], 0.0, np.zeros((4, 2)), 3)
    add("greedy, rejection at row 0", lg, [3, worst[0], best[1], best[2]], 0.0, np.zeros((4, 2)), 0)
    tie = rows(3)
    tie[1, 40] = tie[1, V - 9] = tie[1].max() + F32(1.0)
    add("greedy, the draft on the second of two equal maxima", tie, [3, int(np.argmax(tie[0])), V - 9], 0.0, np.full((3, 2), 2.0), 1)
    lg = rows(2)
    d = V - 3
    pd = float(vr.probs(lg[0], T)[d])
    assert pd > 0
    add("accept coin == p[d]", lg, [5, d], T, [(pd, .5), (.9, .37)], 0)
    add("accept coin one ulp below p[d]", lg, [5, d], T, [(float(np.nextafter(F32(pd), F32(0))), .5), (.9, .37)], 1)
    lg = rows(2)
    lg[0, 9] = lg[0].min() - F32(200.0)
    assert vr.probs(lg[0], T)[9] == 0
    add("p[d] underflowed to 0", lg, [5, 9], T, [(0, .5), (.9, .37)], 0)
    lg = rows(2)
    lg[0] = F32(-500.0)
    lg[0, V // 2] = F32(0.0)
    assert vr.probs(lg[0], T)[V // 2] == 1
    add("p[d] == 1", lg, [5, V // 2], T, [(TOP, .5), (.9, .37)], 1)
    lg = rows(2)
    for d in (0, V - 1):
        lg[0, d] = lg[0].max() + F32(1.0)                  # the likeliest token is the one that must not come back
        for emit in (0.0, 0.5, TOP):
            add("resample with d = %d, emit coin %r" % (d, emit), lg, [5, d], T, [(TOP, emit), (.9, .37)], 0)
    lg = rows(4)
    for i, emit in enumerate((TOP, 0.0, 0.31)):
        add("a run of one row, emit coin %r" % emit, lg[i:i + 1], [7], T, [(.5, emit)], 0)
    add("a greedy run of one row", lg[3:4], [7], 0.0, [(0, 0)], 0)
    return cases


@pytest.mark.parametrize("V", [1008, 4112, 9232])
def test_verify_rows_on_crafted_logits(pkg, planmod, V):
    plan_mod, _ = planmod
    m = pkg.synth.make_numpy(dataclasses.replace(pkg.synth.CONFIGS["tiny-llama"], vocab=V), seed=5)
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=64)
    T = 0.7
    cases = crafted(V, np.random.default_rng(V), T)
    for what, lg, tokens, temp, coins, accepted in cases:
        keep = lg.copy()
        want = vr.verify_rows(lg, tokens, [len(tokens)], [temp], coins)
        assert want[0][0] == accepted, (what, want)                    # the case is what its name says
        if "resample" in what or "underflowed" in what:
            assert want[0][1] != tokens[1], what
        got = plan.verify_rows(lg, tokens, [len(tokens)], [temp], coins)
        assert as_pairs(got) == want, (V, what, as_pairs(got), want)
        assert np.array_equal(lg, keep)
    # every run in one call: greedy and sampled temperatures mixed, runs of 1 .. 4 rows
    lg = np.concatenate([c[1] for c in cases])
    tokens = sum((c[2] for c in cases), [])
    run_rows = [len(c[2]) for c in cases]
    temps = [c[3] * (1.0 + 0.5 * (k % 3)) for k, c in enumerate(cases)]
    coins = np.concatenate([c[4] for c in cases])
    assert lg.shape[0] <= 64 and 0.0 in temps and len({t for t in temps if t > 0}) == 3
    want = vr.verify_rows(lg, tokens, run_rows, temps, coins)
    got = plan.verify_rows(lg, tokens, run_rows, temps, coins)
    assert as_pairs(got) == want, (V, "mixed", as_pairs(got), want)
    greedy_only = [k for k, c in enumerate(cases) if c[3] == 0.0]
    got = plan.verify_rows(np.concatenate([cases[k][1] for k in greedy_only]), sum((cases[k][2] for k in greedy_only), []),
                           [len(cases[k][2]) for k in greedy_only])              # temperature NULL, coins NULL
    assert as_pairs(got) == [want[k] for k in greedy_only]
    plan.freeTornadoExecutionPlan()


@pytest.mark.parametrize("cfg", ["tiny-llama", "tiny-qwen3"])
def test_through_the_forward_pass(pkg, orc, planmod, cfg):
    """Three sequences.  Step 1, greedy: the drafts are the oracle's greedy continuation with one wrong token at row 2 (sequence 0), none
    (sequence 1: every draft stands) and at row 0 (sequence 2).  Step 2: each sequence continues at p + a + 1 with sampled and greedy runs
    whose drafts are again the oracle's; the oracle never saw the rejected drafts, so equal logits show that their K / V rows were
    overwritten before anything read them.  Step 3: one more row per sequence, logits compared."""
    plan_mod, _ = planmod
    m = pkg.synth.make_numpy(pkg.synth.CONFIGS[cfg], seed=97)
    V = m.cfg.vocab
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=32, n_seqs=3)
    oracles = [orc.COracle(m) for _ in range(3)]
    rng = np.random.default_rng(41)
    prompts = [rng.integers(0, V, L).tolist() for L in (6, 3, 9)]
    pos, last = [], []
    for s, p in enumerate(prompts):
        plan.prefill_seq(s, p[:-1], 0); oracles[s].prefill(p[:-1], 0)
        pos.append(len(p) - 1); last.append(p[-1])

    def continuation(s, k):
        """the oracle's logits of k + 1 rows from (last[s], pos[s]) along its own greedy ids -> (logits [k + 1][V], greedy ids [k + 1])"""
        lg, ids, tok = [], [], last[s]
        for i in range(k + 1):
            lg.append(oracles[s].forward(tok, pos[s] + i).copy())
            tok = orc.argmax(lg[-1])
            ids.append(tok)
        return np.stack(lg), ids

    def step(wrong, temps, coins_of):
        """wrong[s]: the row of sequence s whose draft is replaced (None: none), 4 drafts each"""
        toks, seqs, poss, want, coins = [], [], [], [], []
        for s in range(3):
            lg, ids = continuation(s, 4)
            run = [last[s]] + ids[:4]
            if wrong[s] is not None:
                run[wrong[s] + 1] = (ids[wrong[s]] + 1) % V
                # rows behind the wrong draft saw it: the oracle's logits for them are not the step's, and the rule never reads them
            c = coins_of(s)
            want.append(vr.verify_run(lg, run, temps[s], c))
            if temps[s] == 0:
                assert want[-1] == ((wrong[s], ids[wrong[s]]) if wrong[s] is not None else (4, ids[4]))
            toks += run; seqs += [s] * 5; poss += list(range(pos[s], pos[s] + 5)); coins += list(c)
        got = as_pairs(plan.forward_batch_verify(toks, seqs, poss, temps, np.asarray(coins, F32)))
        for s in range(3):
            a, tok = want[s]
            if wrong[s] is not None and temps[s] > 0:
                assert a <= wrong[s]                      # a sampled run may reject earlier, never later than the wrong draft ...
            assert got[s] == want[s], (cfg, s, got, want)
            pos[s] += a + 1; last[s] = tok
        return got

    step([2, None, 0], [0.0, 0.0, 0.0], lambda s: [(0.0, 0.0)] * 5)
    assert pos == [5 + 3, 2 + 5, 8 + 1]
    # ... which needs an accept coin that rejects it: the wrong draft of a sampled run gets the largest coin, the others 0
    top_at = lambda row: [(TOP if i == row else 0.0, 0.42) for i in range(5)]
    step([1, 3, None], [0.8, 0.0, 1.3], lambda s: top_at({0: 1, 1: 0, 2: 9}[s]))
    for s in range(3):
        want = oracles[s].forward(last[s], pos[s])
        got, ids = plan.forward_batch([last[s]], [s], [pos[s]])
        assert np.array_equal(got[0], want), (cfg, s)
        assert int(ids[0]) == orc.argmax(want)
    plan.freeTornadoExecutionPlan()


def test_single_rows_are_the_batched_decode_and_the_batched_sampler(pkg, planmod):
    plan_mod, _ = planmod
    m = pkg.synth.make_numpy(pkg.synth.CONFIGS["tiny-llama"], seed=99)
    V = m.cfg.vocab
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=16, n_seqs=3)
    rng = np.random.default_rng(43)
    for s, L in enumerate((4, 7, 2)):
        plan.prefill_seq(s, rng.integers(0, V, L).tolist(), 0)
    toks, seqs, poss = rng.integers(0, V, 3).tolist(), [2, 0, 1], [2, 4, 7]
    _, ids = plan.forward_decode_batch(toks, seqs, poss, want_logits=False)
    got = plan.forward_batch_verify(toks, seqs, poss)
    assert got["accepted"].tolist() == [0, 0, 0] and got["token"].tolist() == ids.tolist()
    temps, emit = [0.8, 0.0, 1.4], rng.random(3).astype(F32)
    sampled = plan.forward_batch_sample(toks, seqs, poss, temps, 0.0, emit)
    coins = np.stack([rng.random(3).astype(F32), emit], axis=1)
    got = plan.forward_batch_verify(toks, seqs, poss, temps, coins)
    assert got["accepted"].tolist() == [0, 0, 0] and got["token"].tolist() == sampled.tolist()
    assert got["token"][1] == ids[1]
    plan.freeTornadoExecutionPlan()


def test_refusals(pkg, orc, planmod):
    """Every refusal is an argument error raised before anything is enqueued: the KV rows are untouched and the valid step that follows
    matches the CPU oracle bit for bit."""
    plan_mod, hip = planmod
    m = pkg.synth.make_numpy(pkg.synth.CONFIGS["tiny-llama"], seed=93)
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=8, n_seqs=2)
    oracles = [orc.COracle(m) for _ in range(2)]
    rng = np.random.default_rng(31)
    V, ctx = m.cfg.vocab, m.cfg.ctx
    first = rng.integers(0, V, 5).tolist()
    plan.prefill_seq(0, first, 0); oracles[0].prefill(first, 0)
    toks, seqs, poss = rng.integers(0, V, 4).tolist(), [0, 0, 0, 1], [5, 6, 7, 0]
    ok_coins = np.full((4, 2), 0.5, F32)

    def kv_rows():
        return [np.concatenate(plan.kv_seq(s, l, p)) for s, p in ((0, 0), (0, 4), (0, 5), (0, 7), (1, 0)) for l in range(m.cfg.n_layers)]

    def coins_with(row, col, value):
        c = ok_coins.copy()
        c[row, col] = value
        return c
    before = kv_rows()
    nan = float("nan")
    bad_steps = [
        (toks + toks + [1], [0] * 9, list(range(5, 14)), None, None),                      # n > max_batch
        ([V] + toks[1:], seqs, poss, None, None), ([-1] + toks[1:], seqs, poss, None, None),      # what gl3_forward_batch refuses
        (toks, [0, 0, 0, 2], poss, None, None), (toks, seqs, [5, 6, 8, 0], None, None), (toks, [0, 0, 1, 0], [5, 6, 0, 7], None, None),
        (toks, seqs, [ctx - 2, ctx - 1, ctx, 0], None, None), (toks, seqs, [5, 6, 7, -1], None, None),
        (toks, seqs, poss, [-0.5, 0.0], ok_coins), (toks, seqs, poss, [0.0, nan], ok_coins),      # temperature
        (toks, seqs, poss, [0.7, 0.0], None), (toks, seqs, poss, [0.0, 0.7], None),              # coins NULL with a sampled run
        (toks, seqs, poss, [0.7, 0.0], coins_with(1, 0, 1.0)), (toks, seqs, poss, [0.7, 0.0], coins_with(2, 1, -0.25)),
        (toks, seqs, poss, [0.0, 0.7], coins_with(3, 1, nan)),
    ]
    for t, s, p, temps, coins in bad_steps:
        with pytest.raises(hip.Gl3Error) as ei:
            plan.forward_batch_verify(t, s, p, temps, coins)
        assert ei.value.code == hip.E_ARG, (t, s, p, temps)
    L = hip.lib()
    arr = lambda v: np.ascontiguousarray(v, np.int32)
    t_, s_, p_ = arr(toks), arr(seqs), arr(poss)
    res, cnt = np.zeros(4, plan_mod.VERIFY_DTYPE), np.zeros(1, np.int32)
    ptr = lambda a: a.ctypes.data
    cnt_p = cnt.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    assert L.gl3_forward_batch_verify(plan._ctx, ptr(t_), ptr(s_), ptr(p_), 4, None, None, None, cnt_p) == hip.E_ARG
    assert L.gl3_forward_batch_verify(plan._ctx, ptr(t_), ptr(s_), ptr(p_), 4, None, None, ptr(res), None) == hip.E_ARG
    assert L.gl3_forward_batch_verify(plan._ctx, None, ptr(s_), ptr(p_), 4, None, None, ptr(res), cnt_p) == hip.E_ARG
    assert L.gl3_forward_batch_verify(plan._ctx, ptr(t_), ptr(s_), ptr(p_), 0, None, None, ptr(res), cnt_p) == hip.E_ARG
    lg = rng.standard_normal((9, V)).astype(F32)
    bad_rows = [
        (lg[:4], toks, [3, 1], [-0.5, 0.0], ok_coins), (lg[:4], toks, [3, 1], [nan, 0.0], ok_coins), (lg[:4], toks, [3, 1], [0.7, 0.0], None),
        (lg[:4], toks, [3, 1], [0.7, 0.0], coins_with(0, 1, 1.0)), (lg[:4], [V] + toks[1:], [3, 1], None, None),
        (lg[:4], toks[:3] + [-1], [3, 1], None, None), (lg[:4], toks, [4, 0], None, None), (lg, toks + toks + [1], [5, 4], None, None),
    ]
    for rows, t, rr, temps, coins in bad_rows:
        with pytest.raises(hip.Gl3Error) as ei:
            plan.verify_rows(rows, t, rr, temps, coins)
        assert ei.value.code == hip.E_ARG, (t, rr, temps)
    assert L.gl3_verify_rows(plan._ctx, ptr(lg), ptr(t_), ptr(arr([3, 1])), 2, None, None, None) == hip.E_ARG
    assert L.gl3_verify_rows(plan._ctx, ptr(lg), ptr(t_), None, 2, None, None, ptr(res)) == hip.E_ARG
    after = kv_rows()
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    # a coin outside [0, 1) on a GREEDY run is not looked at: the valid step, against the oracle
    got = as_pairs(plan.forward_batch_verify(toks, seqs, poss, [0.0, 0.9], coins_with(1, 0, 7.0)))
    logits = [oracles[s].forward(t, p) for t, s, p in zip(toks, seqs, poss)]
    want = [vr.verify_run(np.stack(logits[:3]), toks[:3]), vr.verify_run(np.stack(logits[3:]), toks[3:], 0.9, ok_coins[3:])]
    assert got == want
    for s, p in ((0, 7), (1, 0)):
        for l in range(m.cfg.n_layers):
            k, v = plan.kv_seq(s, l, p)
            ko, vo = oracles[s].kv(l, p)
            assert np.array_equal(k, ko) and np.array_equal(v, vo)
    plan.freeTornadoExecutionPlan()
    single = plan_mod.HipMasterPlan(m, prefill_batch_size=1)
    with pytest.raises(hip.Gl3Error) as ei:
        single.forward_batch_verify([1], [0], [0])
    assert ei.value.code == hip.E_UNSUPPORTED
    with pytest.raises(hip.Gl3Error) as ei:
        single.verify_rows(lg[:1], [2], [1])
    assert ei.value.code == hip.E_UNSUPPORTED
    single.freeTornadoExecutionPlan()


def test_tensor_parallel_plans_are_refused(pkg, orc, planmod):
    """tp_size > 1 (two ranks as threads on one GPU, max_batch > 1): both entries return GL3_E_UNSUPPORTED on every rank and enqueue nothing —
    the static-batched decode step that follows on both ranks (it needs both: its gathers wait for the peer) equals the oracle bit for bit."""
    import threading
    plan_mod, hip = planmod
    tp, nseq = 2, 3
    m = pkg.synth.make_numpy(pkg.synth.CONFIGS["tiny-llama"], seed=95)
    V = m.cfg.vocab
    rng = np.random.default_rng(47)
    toks = rng.integers(0, V, nseq).tolist()
    lg = rng.standard_normal((3, V)).astype(F32)
    ref = [orc.COracle(m).forward(t, 0) for t in toks]
    grp = plan_mod.make_local_group(tp)
    out, err = [None] * tp, [None] * tp

    def rank_main(r):
        try:
            plan = plan_mod.HipMasterPlan(m, prefill_batch_size=8, n_seqs=nseq, tp_rank=r, tp_size=tp, local_group=grp)
            codes = []
            for call in (lambda: plan.forward_batch_verify([1, 2, 3], [0, 0, 1], [0, 1, 0]),
                         lambda: plan.forward_batch_verify([1, 2, 3], [0, 0, 1], [0, 1, 0], [0.7, 0.0], np.full((3, 2), 0.5, F32)),
                         lambda: plan.forward_batch_verify(toks, [0, 1, 2], [0, 0, 0]),
                         lambda: plan.verify_rows(lg, [1, 2, 3], [2, 1]),
                         lambda: plan.verify_rows(lg, [1, 2, 3], [2, 1], [0.7, 0.0], np.full((3, 2), 0.5, F32))):
                try:
                    call()
                    codes.append(0)
                except hip.Gl3Error as e:
                    codes.append(e.code)
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
        assert codes == [hip.E_UNSUPPORTED] * 5, (r, codes)
        for s in range(nseq):
            assert np.array_equal(logits[s], ref[s]), (r, s)
            assert int(ids[s]) == orc.argmax(ref[s])
