"""gl3_forward_decode_batch_chain and gl3_draft_probs_put_row on the GPU: k static-batched decode steps behind one wait, every row's id handed
to its next step on the device.  The contract is bit equality with k gl3_forward_decode_batch_sample calls (topp 0) over the shrinking row
prefix and, with a target plan, gl3_draft_probs_put_row per row with a slot: two plans of the same model run side by side, one through the
single calls and one through the chain, and ids, probabilities rows, the step's buffers, the attention form of the last step and the K / V
rows of every chained position are compared with np.array_equal on bit patterns — no tolerances anywhere."""
import ctypes as C
import dataclasses
import threading

import numpy as np
import pytest

import __graft_entry__ as ge
import attn_shapes as sh
import moe_shapes as ms

pytestmark = pytest.mark.gpu
F32 = np.float32
F16, Q4_0, Q8_0 = 1, 2, 8          # ggml types of the synthetic models
NSEQ, MAXB = 4, 8


@pytest.fixture(scope="module")
def planmod():
    from importlib import import_module
    ge.load_package()
    return import_module(ge.PKG_NAME + ".plan"), import_module(ge.PKG_NAME + ".hip")


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def rows_of_step(k_rows, j):
    return sum(1 for ki in k_rows if ki > j)


def single_calls(plan, tokens, seqs, pos, k, k_rows, temps, coins, target=None, slots=None):
    """What the chain must equal: k gl3_forward_decode_batch_sample calls (topp 0) over the rows with k_rows[i] > j, each followed by the
    puts of the rows with a slot.  Returns (ids [k][n] with -1 where a row has no step, {(i, j): probabilities row}, attn_rows per step)."""
    n = len(tokens)
    out, probs, forms, t = np.full((k, n), -1, np.int32), {}, [], list(tokens)
    for j in range(k):
        nj = rows_of_step(k_rows, j)
        co = [float(coins[j][i]) if temps[i] > 0 else 0.0 for i in range(nj)]
        ids = plan.forward_decode_batch_sample(t[:nj], seqs[:nj], [p + j for p in pos[:nj]], temps[:nj], 0.0, co)
        forms.append(list(plan.attn_rows()))
        for i in range(nj):
            if temps[i] > 0:
                probs[(i, j)] = plan.sample_probs_row(i)
            if target is not None and slots[i] >= 0:
                target.draft_probs_put_row(slots[i] + j, plan, i)
            t[i] = int(ids[i])
        out[j, :nj] = ids
    return out, probs, forms


def same_state(a, b, hip, cfg, seqs, pos, k_rows, temps, what, f32_rows=False):
    """Everything the chain's contract lists that can be read back: equal on the two plans"""
    k = max(k_rows)
    last = rows_of_step(k_rows, k - 1)
    for i in range(len(seqs)):
        if i < last and temps[i] > 0:
            assert np.array_equal(bits(a.sample_probs_row(i)), bits(b.sample_probs_row(i))), (what, i)
        else:
            for p in (a, b):
                with pytest.raises(hip.Gl3Error):
                    p.sample_probs_row(i)
    q_dim = cfg.n_heads * cfg.head_size
    # 3: the single-token step's logits, which no batched step writes (two_plans ran one such step); 4 .. 6: the rows of the last step (one
    # rank: plain rows; the rows behind them are whatever the allocation held).  5 and 6, the f32 attention output and hb, are written by
    # the F16 / Q4_0 steps; a Q8_0 step of up to 64 rows through attn_head_kernel hands both on quantised and leaves those buffers as allocated
    # (f32_rows "ao": buffer 5 alone — a Q8_0 step whose rows take the per-row attention pair past AF_MAXN writes the f32 attention output)
    for which, n in ((3, cfg.vocab), (4, last * cfg.dim)) + (((5, last * q_dim),) if f32_rows else ()) + (((6, last * cfg.hidden),) if f32_rows is True else ()):
        assert np.array_equal(bits(a.buffer(which, n)), bits(b.buffer(which, n))), (what, which)
    assert list(a.attn_rows()) == list(b.attn_rows()), what
    assert a.topp_counts() == b.topp_counts() == (0, 0), what
    for i, s in enumerate(seqs):
        for p in range(pos[i], pos[i] + k_rows[i]):
            for l in range(cfg.n_layers):
                (ka, va), (kb, vb) = a.kv_seq(s, l, p), b.kv_seq(s, l, p)
                assert ka.any() and np.array_equal(bits(ka), bits(kb)) and np.array_equal(bits(va), bits(vb)), (what, s, l, p)


def draw(rng, k, n):
    return np.asarray([[rng.next_float() for _ in range(n)] for _ in range(k)], F32)


def run_pair(hip, one, chain, cfg, tokens, seqs, pos, k_rows, temps, rng, what, f32_rows=False):
    k, n = max(k_rows), len(tokens)
    sampled = any(t > 0 for t in temps)
    coins = draw(rng, k, n) if sampled else None
    want, _, _ = single_calls(one, tokens, seqs, pos, k, k_rows, temps, coins)
    got = chain.forward_decode_batch_chain(tokens, seqs, pos, k, temps, coins, k_rows if len(set(k_rows)) > 1 else None)
    assert got.dtype == np.int32 and got.shape == (k, n) and np.array_equal(got, want), (what, got, want)
    same_state(one, chain, hip, cfg, seqs, pos, k_rows, temps, what, f32_rows)
    return want


def two_plans(plan_mod, m, flags=0, nseq=NSEQ, maxb=MAXB):
    """Two plans of one model.  Each has run one single-token step (sequence 0, position 0), so that gl3_get_buffer(3) holds that step's
    logits on both and not what the allocation happened to hold."""
    plans = [plan_mod.HipMasterPlan(m, prefill_batch_size=maxb, n_seqs=nseq, flags=flags) for _ in range(2)]
    for p in plans:
        p.forward_decode_argmax(1, 0)
    return plans


def models(pkg):
    c = pkg.synth.CONFIGS
    return {"tiny-llama-q8-graph": (lambda: pkg.synth.make_numpy(c["tiny-llama"], wtype=Q8_0, seed=91), False),
            "tiny-llama-q8-eager": (lambda: pkg.synth.make_numpy(c["tiny-llama"], wtype=Q8_0, seed=91), True),
            "tiny-llama-f16": (lambda: pkg.synth.make_numpy(c["tiny-llama"], wtype=F16, seed=91), False),
            "tiny-llama-q4_0": (lambda: pkg.synth.make_numpy(c["tiny-llama"], wtype=Q4_0, seed=91), False),
            "mid-qwen3-q8": (lambda: pkg.synth.make_numpy(c["mid-qwen3"], wtype=Q8_0, seed=91), False),
            "qwen2moe-e8-k2": (lambda: ms.case_model(pkg, "e8-k2-sh128"), False)}


PATTERNS = {"mixed": [0.8, 0.0, 0.8, 0.0], "greedy": [0.0] * 4, "sampled": [0.8] * 4, "mixed-greedy-first": [0.0, 0.8, 0.8, 0.0]}


@pytest.mark.parametrize("case", ["tiny-llama-q8-graph", "tiny-llama-q8-eager", "tiny-llama-f16", "tiny-llama-q4_0", "mid-qwen3-q8", "qwen2moe-e8-k2"])
def test_chain_equals_the_single_calls(pkg, planmod, case):
    """n in {1, 3, 4} x k in {1, 2, 5}, each with mixed, all-greedy and all-sampled rows, rows at different positions and in an order that is
    not the sequences', one case after the other on the same two plans: every case also checks that the chain left the plan where the single
    calls leave it.  The three settings of a (n, k) start at the same positions (the rows are written again); the next (n, k) goes on behind."""
    plan_mod, hip = planmod
    make, no_graph = models(pkg)[case]
    m = make()
    cfg = m.cfg
    one, chain = two_plans(plan_mod, m, hip.FLAG_NO_GRAPH if no_graph else 0)
    g = np.random.default_rng(92)
    prompts = [g.integers(0, cfg.vocab, n).tolist() for n in (4, 7, 2, 9)]
    for p in (one, chain):
        for s, pr in enumerate(prompts):
            p.prefill_seq(s, pr[:-1], 0)
    rng = pkg.javarand.L32X64MixRandom(1234)
    token = {s: prompts[s][-1] for s in range(NSEQ)}
    at = {s: len(prompts[s]) - 1 for s in range(NSEQ)}
    order = [2, 0, 3, 1]
    names = list(PATTERNS)
    turn = 0
    for n in (1, 3, 4):
        for k in (1, 2, 5):
            seqs = order[:n]
            settings = ["mixed", "greedy", "sampled"] if n > 1 else [names[turn % 3]]      # one row: the three settings by turns
            turn += 1
            for name in settings:
                temps = PATTERNS[name][:n]
                want = run_pair(hip, one, chain, cfg, [token[s] for s in seqs], seqs, [at[s] for s in seqs], [k] * n, temps, rng, (case, n, k, name), m.wtype != Q8_0)
            for i, s in enumerate(seqs):
                token[s], at[s] = int(want[-1, i]), at[s] + k
    assert max(at.values()) < cfg.ctx
    # the plans go on from the same state: one more single batched call on each
    seqs = list(range(NSEQ))
    co = draw(rng, 1, NSEQ)[0]
    args = ([token[s] for s in seqs], seqs, [at[s] for s in seqs], PATTERNS["mixed-greedy-first"], 0.0, co)
    assert np.array_equal(one.forward_decode_batch_sample(*args), chain.forward_decode_batch_sample(*args))
    same_state(one, chain, hip, cfg, seqs, [at[s] for s in seqs], [1] * NSEQ, PATTERNS["mixed-greedy-first"], "single call behind the chains", m.wtype != Q8_0)
    for p in (one, chain):
        p.freeTornadoExecutionPlan()


@pytest.mark.parametrize("pattern", ["mixed", "mixed-greedy-first", "greedy"])
def test_rows_with_fewer_steps(pkg, planmod, pattern):
    """k_rows = (5, 3, 3, 1): the rows of a step are a prefix, ids past a row's last step are -1, K / V is written exactly up to
    positions[i] + k_i - 1 and the row above stays as it was (never written: zero).  With the greedy row first the last two steps run no
    sampler at all, as the single calls."""
    plan_mod, hip = planmod
    cfg = pkg.synth.CONFIGS["tiny-llama"]
    m = pkg.synth.make_numpy(cfg, seed=93)
    one, chain = two_plans(plan_mod, m)
    k_rows, seqs, pos = [5, 3, 3, 1], [1, 3, 0, 2], [0, 2, 1, 3]
    g = np.random.default_rng(94)
    for p in (one, chain):
        for s, at in zip(seqs, pos):
            if at:
                p.prefill_seq(s, g.integers(0, cfg.vocab, at).tolist(), 0)
        g = np.random.default_rng(94)
    got = run_pair(hip, one, chain, cfg, [5, 6, 7, 8], seqs, pos, k_rows, PATTERNS[pattern], pkg.javarand.L32X64MixRandom(3), pattern)
    for i, ki in enumerate(k_rows):
        assert (got[:ki, i] >= 0).all() and (got[ki:, i] == -1).all(), (i, got)
        for l in range(cfg.n_layers):
            for p in (one, chain):
                ka, va = p.kv_seq(seqs[i], l, pos[i] + ki)
                assert not ka.any() and not va.any(), (i, l)
    for p in (one, chain):
        p.freeTornadoExecutionPlan()


@pytest.mark.parametrize("no_graph", [False, True], ids=["graph", "eager"])
def test_a_chain_crosses_the_attention_regime(pkg, planmod, no_graph):
    """Two rows, one 3 positions below AF_MAXN and one at position 2, k = 6: the deepest row leaves attn_head_kernel's range inside the chain,
    so the step changes from the captured replay (or its eager launches) to the per-row pair.  The reference plan's gl3_get_attn_rows says
    so for a step before and a step after."""
    plan_mod, hip = planmod
    K = 6
    cfg = dataclasses.replace(pkg.synth.CONFIGS["tiny-llama"], ctx=(sh.AF_MAXN + 3 + 3) & ~3)
    assert cfg.ctx >= sh.AF_MAXN + 3
    m = pkg.synth.make_numpy(cfg, seed=95)
    one, chain = two_plans(plan_mod, m, hip.FLAG_NO_GRAPH if no_graph else 0, nseq=2, maxb=64)
    deep = sh.AF_MAXN - 3
    prompt = np.random.default_rng(96).integers(0, cfg.vocab, deep + 1).tolist()
    for p in (one, chain):
        p.prefill_seq(0, prompt[:deep], 0)
        p.prefill_seq(1, prompt[:2], 0)
    seqs, pos, k_rows, rng = [0, 1], [deep, 2], [K, K], pkg.javarand.L32X64MixRandom(5)
    for temps in ([0.8, 0.0], [0.0, 0.0]):                               # the greedy chain runs over the same positions again
        coins = draw(rng, K, 2) if any(temps) else None
        want, _, forms = single_calls(one, [prompt[deep], prompt[2]], seqs, pos, K, k_rows, temps, coins)
        assert forms[0] == sh.batched_rows(cfg.head_size, [deep, 2]) == [2, 0, 0, 0], forms
        assert forms[-1] == sh.batched_rows(cfg.head_size, [deep + K - 1, 2 + K - 1]) == [0, 0, 0, 2] and forms[2] != forms[3], forms
        got = chain.forward_decode_batch_chain([prompt[deep], prompt[2]], seqs, pos, K, temps, coins)
        assert np.array_equal(got, want), (temps, got, want)
        same_state(one, chain, hip, cfg, seqs, pos, k_rows, temps, (no_graph, temps), "ao")      # the last step took the pair: AO is written
    for p in (one, chain):
        p.freeTornadoExecutionPlan()


def test_chain_fills_the_targets_draft_table(pkg, planmod):
    """Every slot slots[i] + j of the target equals the single-call plan's sample_probs_row(i) after step j and what gl3_draft_probs_put_row
    left in a second target; a greedy row (slot -1) writes nothing; slots around them keep what they held; the two targets decide a
    verification step alike."""
    plan_mod, hip = planmod
    cfg = pkg.synth.CONFIGS["tiny-llama"]
    tm = pkg.synth.make_numpy(cfg, seed=97)
    dm = pkg.synth.make_numpy(dataclasses.replace(cfg, n_layers=1), seed=98)
    targets, drafts = two_plans(plan_mod, tm), two_plans(plan_mod, dm)
    prompt = np.random.default_rng(99).integers(0, cfg.vocab, 6).tolist()
    for p in targets + drafts:
        for s in range(3):
            p.prefill_seq(s, prompt[s:-1], 0)
    seqs, pos = [0, 1, 2], [5, 4, 3]
    k, k_rows, temps, slots = 2, [2, 2, 1], [0.8, 0.0, 0.8], [1, -1, 5]
    rng = pkg.javarand.L32X64MixRandom(7)
    coins = draw(rng, k, 3)
    below = np.random.default_rng(100).random(cfg.vocab).astype(F32)
    for t in targets:
        t.draft_probs_put_host(0, below)
    tokens = [prompt[-1]] * 3
    want, probs, _ = single_calls(drafts[0], tokens, seqs, pos, k, k_rows, temps, coins, targets[0], slots)
    got = drafts[1].forward_decode_batch_chain(tokens, seqs, pos, k, temps, coins, k_rows, targets[1], slots)
    assert np.array_equal(got, want)
    same_state(drafts[0], drafts[1], hip, dm.cfg, seqs, pos, k_rows, temps, "draft plans")
    written = {1: (0, 0), 2: (0, 1), 5: (2, 0)}                           # slot -> (row, step)
    for slot, (i, j) in written.items():
        row = targets[1].draft_probs(slot)
        assert np.array_equal(bits(row), bits(probs[(i, j)])) and np.array_equal(bits(row), bits(targets[0].draft_probs(slot))), slot
    assert not np.array_equal(targets[1].draft_probs(1), targets[1].draft_probs(2))      # one row per step, not the last one twice
    for t in targets:
        assert np.array_equal(bits(t.draft_probs(0)), bits(below))
        for slot in (3, 4, 6, 7):
            with pytest.raises(hip.Gl3Error) as ei:
                t.draft_probs(slot)
            assert ei.value.code == hip.E_STATE
    # row 0 of the chain's last step may be put again by hand, as after the single calls
    targets[1].draft_probs_put_row(7, drafts[1], 0)
    assert np.array_equal(bits(targets[1].draft_probs(7)), bits(probs[(0, 1)]))
    toks = [prompt[-1]] + want[:, 0].tolist()
    vcoins = np.asarray([rng.next_float() for _ in range(2 * (k + 1))], F32).reshape(k + 1, 2)
    res = [t.forward_batch_verify_dist(toks, [0] * (k + 1), list(range(pos[0], pos[0] + k + 1)), [0.8], vcoins, [1, 2, -1]) for t in targets]
    assert len(res[0]) == 1 and res[0].tolist() == res[1].tolist()
    for p in targets + drafts:
        p.freeTornadoExecutionPlan()


def test_chain_ids_are_the_oracle_sampler_loop(pkg, orc, planmod):
    plan_mod, _ = planmod
    cfg = pkg.synth.CONFIGS["tiny-llama"]
    m = pkg.synth.make_numpy(cfg, seed=101)
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=MAXB, n_seqs=2)
    g = np.random.default_rng(102)
    prompts = [g.integers(0, cfg.vocab, n).tolist() for n in (6, 3)]
    oracles = [orc.COracle(m) for _ in range(2)]
    for s, pr in enumerate(prompts):
        plan.prefill_seq(s, pr[:-1], 0)
        for p, t in enumerate(pr[:-1]):
            oracles[s].forward(t, p)
    rng = pkg.javarand.L32X64MixRandom(1234)
    k, T = 3, 0.8
    coins = draw(rng, k, 2)
    want, last = np.zeros((k, 2), np.int32), [None, None]
    for s, pr in enumerate(prompts):
        token = pr[-1]
        for j in range(k):
            token, last[s] = orc.sample(oracles[s].forward(token, len(pr) - 1 + j), T, 0.0, float(coins[j][s]), want_probs=True)
            want[j, s] = token
    got = plan.forward_decode_batch_chain([pr[-1] for pr in prompts], [0, 1], [len(pr) - 1 for pr in prompts], k, T, coins)
    assert np.array_equal(got, want) and len(set(want.ravel().tolist())) > 1
    for s in range(2):
        assert np.array_equal(bits(plan.sample_probs_row(s)), bits(last[s]))
    plan.freeTornadoExecutionPlan()


def test_chains_of_chain_max(pkg, planmod):
    """GL3_CHAIN_MAX steps of one row and of two rows on a context of 68 fill the device lists to their last entry."""
    plan_mod, hip = planmod
    k = hip.CHAIN_MAX
    cfg = dataclasses.replace(pkg.synth.CONFIGS["tiny-llama"], ctx=68)
    m = pkg.synth.make_numpy(cfg, seed=103)
    one, chain = two_plans(plan_mod, m, nseq=2)
    rng = pkg.javarand.L32X64MixRandom(11)
    run_pair(hip, one, chain, cfg, [5], [1], [0], [k], [0.8], rng, "one row")
    run_pair(hip, one, chain, cfg, [5, 9], [0, 1], [4, 3], [k, k], [0.0, 0.8], rng, "two rows")
    for p in (one, chain):
        p.freeTornadoExecutionPlan()


def raw_plan(hip, m, max_batch):
    """A plan that gl3_create made and gl3_finalize has not seen"""
    c = m.cfg
    d = hip.ModelDesc(C.sizeof(hip.ModelDesc), c.arch, c.dim, c.hidden, c.n_layers, c.n_heads, c.n_kv_heads, c.head_size, c.vocab, c.ctx,
                      c.rms_eps, m.wtype, max_batch, 0, 0, 1, 0, 1, 1.0, 0.0, 1.0, 1.0, 0, 0, 0)
    raw = C.c_void_p()
    hip.check(hip.lib().gl3_create(C.byref(d), C.byref(raw)))
    return raw


def ptr(a, dtype):
    return np.ascontiguousarray(a, dtype).ctypes.data_as(C.c_void_p) if a is not None else None


def test_refusals(pkg, planmod):
    """Every code the header lists for gl3_forward_decode_batch_chain, each before anything is uploaded or enqueued: after the refused calls a
    K / V row, the probabilities row and the target's table are what they were, and a valid call still equals the single calls.  (Plans on
    different devices need two devices: that refusal cannot be exercised on one and is not exercised here.  tp_size > 1:
    test_tensor_parallel_plans_are_refused below.)"""
    plan_mod, hip = planmod
    L = hip.lib()
    cfg = pkg.synth.CONFIGS["tiny-llama"]
    m = pkg.synth.make_numpy(cfg, seed=105)
    V, ctx = cfg.vocab, cfg.ctx
    one, plan = two_plans(plan_mod, m)
    target = plan_mod.HipMasterPlan(m, prefill_batch_size=MAXB)
    single = plan_mod.HipMasterPlan(m)                                   # max_batch <= 1: no batched step, no draft table
    other_vocab = plan_mod.HipMasterPlan(pkg.synth.make_numpy(dataclasses.replace(cfg, vocab=1008), seed=106), prefill_batch_size=MAXB)
    prompt = np.random.default_rng(107).integers(0, V, 6).tolist()
    for p in (one, plan):
        for s in range(2):
            p.prefill_seq(s, prompt, 0)
        p.forward_decode_batch_sample([prompt[-1]] * 2, [0, 1], [5, 5], 0.8, 0.0, [0.25, 0.5])
    target.draft_probs_put_host(2, np.random.default_rng(108).random(V).astype(F32))
    out = np.zeros((hip.CHAIN_MAX + 1) * MAXB, np.int32)
    good = np.full((4, 2), 0.5, F32)

    def state():
        return [np.concatenate(plan.kv_seq(s, l, p)) for s in (0, 1) for l in range(cfg.n_layers) for p in (0, 5, 6)] + \
               [plan.sample_probs_row(0), plan.sample_probs_row(1), target.draft_probs(2)]

    def call(c, tokens=(3, 4), seqs=(0, 1), pos=(6, 6), n=2, k=2, k_rows=None, temps=(0.0, 0.0), coins=None, tgt=None, slots=None, res=out):
        return L.gl3_forward_decode_batch_chain(c, ptr(tokens, np.int32), ptr(seqs, np.int32), ptr(pos, np.int32), n, k, ptr(k_rows, np.int32),
                                                ptr(temps, F32), ptr(coins, F32), tgt, ptr(slots, np.int32), ptr(res, np.int32))
    before = state()
    assert not before[2].any()                                           # position 6 has not been written: a refused chain must not write it
    P, T_ = plan._ctx, target._ctx
    S = dict(temps=(0.8, 0.8), coins=good)                               # a sampled call that is fine without a target
    nan = float("nan")
    arg = [dict(c=None), dict(c=P, tokens=None), dict(c=P, seqs=None), dict(c=P, pos=None), dict(c=P, temps=None), dict(c=P, res=None),
           dict(c=P, n=0), dict(c=P, n=-1), dict(c=P, n=MAXB + 1, tokens=[3] * 9, seqs=list(range(9)), pos=[6] * 9, temps=[0.0] * 9),
           dict(c=P, k=0), dict(c=P, k=-1), dict(c=P, k=hip.CHAIN_MAX + 1, pos=(0, 0)),
           dict(c=P, k=3, k_rows=(2, 3)), dict(c=P, k=3, k_rows=(2, 2)), dict(c=P, k=3, k_rows=(3, 0)), dict(c=P, k=3, k_rows=(3, 4)),
           dict(c=P, k=3, k_rows=(3, -1)), dict(c=P, n=3, k=3, k_rows=(3, 1, 2), tokens=(3, 4, 5), seqs=(0, 1, 2), pos=(6, 6, 0), temps=(0.0,) * 3),
           dict(c=P, tokens=(-1, 4)), dict(c=P, tokens=(3, V)), dict(c=P, seqs=(0, -1)), dict(c=P, seqs=(0, NSEQ)), dict(c=P, seqs=(1, 1)),
           dict(c=P, pos=(-1, 6)), dict(c=P, pos=(6, ctx - 1)), dict(c=P, pos=(ctx, 6), k=1), dict(c=P, k=3, k_rows=(3, 2), pos=(6, ctx - 1)),
           dict(c=P, temps=(-0.5, 0.0), coins=good), dict(c=P, temps=(0.0, nan), coins=good),
           dict(c=P, temps=(0.8, 0.0)), dict(c=P, temps=(0.0, 0.8), coins=[[0.5, 0.5], [0.5, 1.0]]), dict(c=P, **{**S, "coins": [[-0.1, 0.5], [0.5, 0.5]]}),
           dict(c=P, **{**S, "coins": [[0.5, 0.5], [nan, 0.5]]}),
           dict(c=P, tgt=P, slots=(0, 2), **S), dict(c=P, tgt=T_, slots=None, **S),
           dict(c=P, tgt=T_, slots=(-2, 2), **S), dict(c=P, tgt=T_, slots=(0, MAXB - 1), **S), dict(c=P, tgt=T_, slots=(MAXB, -1), **S),
           dict(c=P, tgt=T_, slots=(0, 1), **S), dict(c=P, tgt=T_, slots=(3, 2), **S), dict(c=P, tgt=T_, slots=(4, 4), **S),
           dict(c=P, tgt=other_vocab._ctx, slots=(0, 2), **S)]
    for a in arg:
        assert call(**a) == hip.E_ARG, a
        assert a["c"] is None or L.gl3_last_error(a["c"]), a
    assert call(P, temps=(0.0, 0.8), tgt=T_, slots=(0, 2)) == hip.E_ARG                                      # (coins NULL with a sampled row)
    assert call(P, temps=(0.0, 0.8), coins=good, tgt=T_, slots=(0, -1)) == hip.E_STATE                       # a greedy row with a slot
    assert call(P, tgt=T_, slots=(0, 2)) == hip.E_STATE
    assert call(P, tgt=single._ctx, slots=(0, 2), **S) == hip.E_UNSUPPORTED
    assert call(single._ctx, seqs=(0, 0), n=1) == hip.E_UNSUPPORTED
    for mb, as_target in ((MAXB, False), (MAXB, True)):                  # before gl3_finalize: the chaining plan, then the target
        raw = raw_plan(hip, m, mb)
        try:
            code = call(P, tgt=raw, slots=(0, 2), **S) if as_target else call(raw)
            assert code == hip.E_STATE, (as_target, code)
        finally:
            L.gl3_destroy(raw)
    with pytest.raises(hip.Gl3Error) as ei:
        plan.forward_decode_batch_chain([3, 4], [0, 1], [6, 6], 2, 0.8, None)
    assert ei.value.code == hip.E_ARG
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(before, state()))
    for s in (0, 1, 3):
        with pytest.raises(hip.Gl3Error) as ei:
            target.draft_probs(s)
        assert ei.value.code == hip.E_STATE
    # the edges that are valid, and equal to the single calls: the last positions of the context (the second row ends inside it through
    # k_rows, positions + k would not), a coin outside [0, 1) on a greedy row, the last slots of the table
    rng = pkg.javarand.L32X64MixRandom(13)
    run_pair(hip, one, plan, cfg, [3, 4], [0, 1], [ctx - 3, ctx - 1], [3, 1], [0.8, 0.8], rng, "context edge")
    coins = np.asarray([[0.5, 7.0], [0.25, 7.0]], F32)
    got = plan.forward_decode_batch_chain([3, 4], [0, 1], [6, 6], 2, [0.8, 0.0], coins, None, target, [MAXB - 2, -1])
    want, probs, _ = single_calls(one, [3, 4], [0, 1], [6, 6], 2, [2, 2], [0.8, 0.0], coins)
    assert np.array_equal(got, want) and np.array_equal(bits(target.draft_probs(MAXB - 1)), bits(probs[(0, 1)]))
    for p in (one, plan, target, single, other_vocab):
        p.freeTornadoExecutionPlan()


def test_put_row_refusals_and_bit_equality(pkg, planmod):
    plan_mod, hip = planmod
    L = hip.lib()
    cfg = pkg.synth.CONFIGS["tiny-llama"]
    m = pkg.synth.make_numpy(cfg, seed=109)
    draft = plan_mod.HipMasterPlan(m, prefill_batch_size=MAXB, n_seqs=NSEQ)
    target = plan_mod.HipMasterPlan(m, prefill_batch_size=MAXB)
    single = plan_mod.HipMasterPlan(m)
    other_vocab = plan_mod.HipMasterPlan(pkg.synth.make_numpy(dataclasses.replace(cfg, vocab=1008), seed=110), prefill_batch_size=MAXB)
    D, T_ = draft._ctx, target._ctx
    assert L.gl3_draft_probs_put_row(T_, 0, D, 0) == hip.E_STATE         # no batched sampled step yet
    draft.forward_decode_batch_sample([3, 4, 5], [0, 1, 2], [0, 0, 0], [0.8, 0.0, 0.7], [0.0, 0.0, 0.9], [0.5, 0.5, 0.5])
    for a in ((None, 0, D, 0), (T_, 0, None, 0), (T_, 0, T_, 0), (T_, -1, D, 0), (T_, MAXB, D, 0), (T_, 0, D, -1), (T_, 0, D, 3), (other_vocab._ctx, 0, D, 0)):
        assert L.gl3_draft_probs_put_row(*a) == hip.E_ARG, a
    assert L.gl3_draft_probs_put_row(T_, 0, D, 1) == hip.E_STATE         # the row was greedy
    assert L.gl3_draft_probs_put_row(T_, 0, D, 2) == hip.E_STATE         # the row went through top-p
    assert L.gl3_draft_probs_put_row(single._ctx, 0, D, 0) == hip.E_UNSUPPORTED
    raw = raw_plan(hip, m, MAXB)
    try:
        assert L.gl3_draft_probs_put_row(raw, 0, D, 0) == hip.E_STATE
    finally:
        L.gl3_destroy(raw)
    for s in range(MAXB):
        with pytest.raises(hip.Gl3Error) as ei:
            target.draft_probs(s)
        assert ei.value.code == hip.E_STATE
    target.draft_probs_put_row(MAXB - 1, draft, 0)
    assert np.array_equal(bits(target.draft_probs(MAXB - 1)), bits(draft.sample_probs_row(0)))
    # a gl3_sample_rows call is a batched sampled step too; the draft goes on sampling behind the copy
    logits = np.random.default_rng(111).standard_normal((2, cfg.vocab)).astype(F32)
    draft.sample_rows(logits, [0.9, 0.6], [0.0, 0.0], [0.3, 0.6])
    row = draft.sample_probs_row(1)
    target.draft_probs_put_row(0, draft, 1)
    draft.sample_rows(logits[::-1], [0.9, 0.6], [0.0, 0.0], [0.3, 0.6])
    assert np.array_equal(bits(target.draft_probs(0)), bits(row)) and not np.array_equal(row, draft.sample_probs_row(1))
    draft.forward_decode_batch_sample([3], [0], [1], 0.0, 0.0, 0.0)        # an all-greedy step: no rows
    assert L.gl3_draft_probs_put_row(T_, 1, D, 0) == hip.E_STATE
    for p in (draft, target, single, other_vocab):
        p.freeTornadoExecutionPlan()


def test_tensor_parallel_plans_are_refused(pkg, orc, planmod):
    """tp_size > 1 (two ranks as threads on one GPU): GL3_E_UNSUPPORTED from gl3_forward_decode_batch_chain on every rank's plan and with a
    rank's plan as the target of a one-rank plan's chain, and from gl3_draft_probs_put_row with a rank's plan as target and as draft.  Nothing
    is enqueued or changed: the one-rank plan keeps its probabilities row and writes no K / V, and the static-batched step that follows on
    both ranks equals the oracle bit for bit."""
    plan_mod, hip = planmod
    tp, nseq = 2, 3
    cfg = pkg.synth.CONFIGS["tiny-llama"]
    m = pkg.synth.make_numpy(cfg, seed=113)
    toks = np.random.default_rng(114).integers(0, cfg.vocab, nseq).tolist()
    ref = [orc.COracle(m).forward(t, 0) for t in toks]
    one_rank = plan_mod.HipMasterPlan(m, prefill_batch_size=MAXB, n_seqs=2)
    one_rank.forward_decode_batch_sample([3, 4], [0, 1], [0, 0], 0.9, 0.0, [0.5, 0.25])
    row = one_rank.sample_probs_row(1)
    grp = plan_mod.make_local_group(tp)
    out, err = [None] * tp, [None] * tp
    co = np.full((2, 2), 0.5, F32)
    sync = threading.Barrier(tp)
    lock = threading.Lock()

    def rank_main(r):
        try:
            plan = plan_mod.HipMasterPlan(m, prefill_batch_size=MAXB, n_seqs=nseq, tp_rank=r, tp_size=tp, local_group=grp)
            calls = [lambda: plan.forward_decode_batch_chain([3, 4], [0, 1], [0, 0], 2, 0.0),
                     lambda: plan.forward_decode_batch_chain([3, 4], [0, 1], [0, 0], 2, 0.8, co),
                     lambda: one_rank.forward_decode_batch_chain([3, 4], [0, 1], [1, 1], 2, 0.8, co, None, plan, [0, 2]),
                     lambda: plan.draft_probs_put_row(0, one_rank, 1),
                     lambda: one_rank.draft_probs_put_row(0, plan, 0)]
            codes = []
            for call in calls:
                try:
                    with lock:                                           # one_rank is shared by the two threads
                        call()
                    codes.append(0)
                except hip.Gl3Error as e:
                    codes.append(e.code)
            sync.wait(timeout=120)       # the one-rank plan goes before the step: the ranks' polling gathers keep the hardware queues to themselves
            if r == 0:
                assert np.array_equal(bits(one_rank.sample_probs_row(1)), bits(row)) and not one_rank.kv_seq(0, 0, 1)[0].any()
                with pytest.raises(hip.Gl3Error):
                    one_rank.draft_probs(0)
                one_rank.freeTornadoExecutionPlan()
            sync.wait(timeout=120)
            out[r] = (codes, plan.forward_decode_batch(toks, [0, 1, 2], [0, 0, 0]))
            plan.freeTornadoExecutionPlan()
        except Exception as e:   # noqa: BLE001
            err[r] = e
            sync.abort()

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
