"""gl3_forward_decode_chain on the GPU: k single-token steps behind one wait, the id each step draws handed to the next on the device.  Its
contract is bit equality with k gl3_forward_decode_sample calls (topp 0) and, with a target plan, k gl3_draft_probs_put: two plans of the same
model run side by side, one through the single calls and one through the chain, and ids, probabilities row, x, the step's buffers and the
K / V rows of every chained position are compared with np.array_equal — at every k, greedy and sampled, captured graph and launch by launch,
across the positions at which the host picks another attention regime, against the CPU oracle's sampler loop, into a target's draft table,
and at GL3_CHAIN_MAX.  Every refusal leaves the plan as it was."""
import ctypes as C
import dataclasses
import threading

import numpy as np
import pytest

import __graft_entry__ as ge
import attn_shapes as sh

pytestmark = pytest.mark.gpu
F32 = np.float32
F16, Q4_0, Q8_0 = 1, 2, 8          # ggml types of the synthetic models


@pytest.fixture(scope="module")
def planmod():
    from importlib import import_module
    ge.load_package()
    return import_module(ge.PKG_NAME + ".plan"), import_module(ge.PKG_NAME + ".hip")


def single_calls(plan, token, pos, k, T, coins, target=None, slot0=0):
    """What the chain must equal: k gl3_forward_decode_sample calls (topp 0), each followed by the put when there is a target"""
    ids = []
    for j in range(k):
        token = plan.forward_decode_sample(token, pos + j, T, 0.0, float(coins[j]) if T > 0 else 0.0)
        if target is not None:
            target.draft_probs_put(slot0 + j, plan)
        ids.append(token)
    return np.asarray(ids, np.int32)


def same_state(a, b, cfg, positions, sampled, what):
    """Everything gl3_forward_decode_chain's contract lists that can be read back: equal on the two plans"""
    if sampled:
        assert np.array_equal(a.sample_probs().view(np.uint32), b.sample_probs().view(np.uint32)), what
    assert np.array_equal(a.x().view(np.uint32), b.x().view(np.uint32)), what
    q_dim = cfg.n_heads * cfg.head_size
    for which, n in ((0, q_dim + 2 * cfg.kv_dim), (1, q_dim), (2, cfg.hidden), (3, cfg.vocab)):
        assert np.array_equal(a.buffer(which, n).view(np.uint32), b.buffer(which, n).view(np.uint32)), (what, which)
    for p in positions:
        for l in range(cfg.n_layers):
            (ka, va), (kb, vb) = a.kv(l, p), b.kv(l, p)
            assert ka.any() and np.array_equal(ka.view(np.uint32), kb.view(np.uint32)) and np.array_equal(va.view(np.uint32), vb.view(np.uint32)), (what, l, p)


def run_pair(pkg, one, chain, cfg, token, pos, k, T, rng, what):
    coins = np.asarray([rng.next_float() for _ in range(k)], F32) if T > 0 else None
    want = single_calls(one, token, pos, k, T, coins)
    got = chain.forward_decode_chain(token, pos, k, T, coins)
    assert got.dtype == np.int32 and np.array_equal(got, want), (what, got, want)
    same_state(one, chain, cfg, range(pos, pos + k), T > 0, what)
    return int(want[-1])


CASES = [("tiny-llama", Q8_0, False), ("tiny-llama", Q8_0, True), ("tiny-llama", F16, False), ("tiny-llama", Q4_0, False),
         ("mid-qwen3", Q8_0, False), ("mid-qwen3", Q8_0, True)]


@pytest.mark.parametrize("name,wtype,no_graph", CASES, ids=["%s-w%d-%s" % (n, w, "eager" if g else "graph") for n, w, g in CASES])
def test_chain_equals_the_single_calls(pkg, planmod, name, wtype, no_graph):
    """k in {1, 2, 5}, greedy and T = 0.8, one case after the other on the same two plans (the chain of a case starts on the id the last one
    ended with, behind its positions), so every case also checks that the chain left the plan where the single calls leave it."""
    plan_mod, hip = planmod
    cfg = pkg.synth.CONFIGS[name]
    m = pkg.synth.make_numpy(cfg, wtype=wtype, seed=71)
    flags = hip.FLAG_NO_GRAPH if no_graph else 0
    one, chain = plan_mod.HipMasterPlan(m, flags=flags), plan_mod.HipMasterPlan(m, flags=flags)
    prompt = np.random.default_rng(72).integers(0, cfg.vocab, 5).tolist()
    for p in (one, chain):
        p.prefill(prompt[:-1], 0)
    rng = pkg.javarand.L32X64MixRandom(1234)
    token, pos = prompt[-1], len(prompt) - 1
    for T in (0.8, 0.0, 0.8):                      # a sampled chain behind a greedy one and the other way round
        for k in (1, 2, 5):
            token = run_pair(pkg, one, chain, cfg, token, pos, k, T, rng, (name, wtype, no_graph, T, k))
            pos += k
    assert pos <= cfg.ctx
    # the plans go on from the same state: one more single call on each
    coin = rng.next_float()
    assert one.forward_decode_sample(token, pos, 0.8, 0.0, coin) == chain.forward_decode_sample(token, pos, 0.8, 0.0, coin)
    same_state(one, chain, cfg, [pos], True, "single call behind the chains")
    for p in (one, chain):
        p.freeTornadoExecutionPlan()


def regime(hip, cfg, pos):
    """AttnRegime of a single-token step of a one-rank plan of `cfg` at `pos`, from the library's own decode attention plan"""
    r, n = C.c_int32(-1), C.c_int32(-1)
    launches, head = np.full((4, 6), -7, np.int64), np.full(3, -7, np.int64)
    code = hip.lib().gl3_debug_decode_attn_plan(cfg.head_size, cfg.n_heads // cfg.n_kv_heads, cfg.n_heads, cfg.n_kv_heads, cfg.ctx, min((cfg.ctx + 3) & ~3, 16384),
                                                sh.ATTN_MID, int(sh.has_head_kernel(cfg.head_size)), pos, 1, C.byref(r), launches.ctypes.data_as(C.c_void_p),
                                                C.byref(n), head.ctypes.data_as(C.c_void_p))
    assert code == 0
    return r.value


@pytest.mark.parametrize("no_graph", [False, True], ids=["graph", "eager"])
def test_a_chain_crosses_the_attention_regimes(pkg, planmod, no_graph):
    """A chain of 6 that starts 3 positions below 128 and one that starts 3 below the two-launch limit: which captured step is replayed, and
    which attention kernels a step launches, changes inside the chain.  Both limits come from gl3_debug_decode_attn_plan on the plan's own
    numbers, and the regimes at the first and the last chained position differ, or the test would show nothing."""
    plan_mod, hip = planmod
    K = 6
    base = pkg.synth.CONFIGS["tiny-llama"]
    probe = dataclasses.replace(base, ctx=4096)
    codes = [regime(hip, probe, p) for p in range(2048)]
    long_from = codes.index(0)                                           # ATT_LONG: past the two-launch pair
    short_to = max(p for p, c in enumerate(codes) if c == 1) + 1         # ATT_SHORT: attn_head_kernel
    assert (short_to, long_from) == (sh.AF_MAXN, sh.ATTN_MID)
    cfg = dataclasses.replace(base, ctx=(long_from + K - 3 + 3) & ~3)    # just long enough, a multiple of 4 for the batched prefill
    m = pkg.synth.make_numpy(cfg, seed=73)
    flags = hip.FLAG_NO_GRAPH if no_graph else 0
    one, chain = (plan_mod.HipMasterPlan(m, prefill_batch_size=64, flags=flags) for _ in range(2))
    prompt = np.random.default_rng(74).integers(0, cfg.vocab, cfg.ctx).tolist()
    rng = pkg.javarand.L32X64MixRandom(5)
    done = 0
    for start in (short_to - 3, long_from - 3):
        assert start + K <= cfg.ctx
        first, last = regime(hip, cfg, start), regime(hip, cfg, start + K - 1)
        assert first != last, (start, first, last)
        for p in (one, chain):
            p.prefill(prompt[done:start], done)
        for T in (0.8, 0.0):                                             # the greedy chain runs over the same positions again
            run_pair(pkg, one, chain, cfg, prompt[start], start, K, T, rng, (no_graph, start, T))
        done = start + K
    for p in (one, chain):
        p.freeTornadoExecutionPlan()


def test_chain_ids_are_the_oracle_sampler_loop(pkg, orc, planmod):
    plan_mod, _ = planmod
    cfg = pkg.synth.CONFIGS["tiny-llama"]
    m = pkg.synth.make_numpy(cfg, seed=75)
    plan, o = plan_mod.HipMasterPlan(m), orc.COracle(m)
    prompt = np.random.default_rng(76).integers(0, cfg.vocab, 6).tolist()
    plan.prefill(prompt[:-1], 0)
    o.prefill(prompt[:-1], 0)
    rng = pkg.javarand.L32X64MixRandom(1234)
    k, T = 8, 0.8
    coins = np.asarray([rng.next_float() for _ in range(k)], F32)
    want, token, probs = [], prompt[-1], None
    for j in range(k):
        token, probs = orc.sample(o.forward(token, len(prompt) - 1 + j), T, 0.0, float(coins[j]), want_probs=True)
        want.append(token)
    got = plan.forward_decode_chain(prompt[-1], len(prompt) - 1, k, T, coins)
    assert got.tolist() == want and len(set(want)) > 1
    assert np.array_equal(plan.sample_probs().view(np.uint32), np.asarray(probs, F32).view(np.uint32))
    plan.freeTornadoExecutionPlan()


def test_chain_fills_the_targets_draft_table(pkg, planmod):
    """Slots slot0 .. slot0 + k - 1 of the target equal what the single calls with gl3_draft_probs_put leave in a second target, the slots on
    both sides of them keep what they held, and the two targets decide a verification step alike."""
    plan_mod, hip = planmod
    cfg = pkg.synth.CONFIGS["tiny-llama"]
    tm = pkg.synth.make_numpy(cfg, seed=77)
    dm = pkg.synth.make_numpy(dataclasses.replace(cfg, n_layers=1), seed=78)
    targets = [plan_mod.HipMasterPlan(tm, prefill_batch_size=8) for _ in range(2)]
    drafts = [plan_mod.HipMasterPlan(dm) for _ in range(2)]
    prompt = np.random.default_rng(79).integers(0, cfg.vocab, 6).tolist()
    for p in targets + drafts:
        p.prefill(prompt[:-1], 0)
    k, slot0, T, pos = 3, 1, 0.8, len(prompt) - 1
    rng = pkg.javarand.L32X64MixRandom(7)
    coins = np.asarray([rng.next_float() for _ in range(k)], F32)
    below = np.random.default_rng(80).random(cfg.vocab).astype(F32)
    for t in targets:
        t.draft_probs_put_host(0, below)
    want = single_calls(drafts[0], prompt[-1], pos, k, T, coins, targets[0], slot0)
    got = drafts[1].forward_decode_chain(prompt[-1], pos, k, T, coins, targets[1], slot0)
    assert np.array_equal(got, want)
    same_state(drafts[0], drafts[1], dm.cfg, range(pos, pos + k), True, "draft plans")
    rows = [targets[1].draft_probs(slot0 + j) for j in range(k)]
    for j in range(k):
        assert np.array_equal(rows[j].view(np.uint32), targets[0].draft_probs(slot0 + j).view(np.uint32)), j
    assert np.array_equal(rows[-1].view(np.uint32), drafts[1].sample_probs().view(np.uint32))
    assert not np.array_equal(rows[0], rows[1])                          # one row per step, not the last one k times
    for t in targets:
        assert np.array_equal(t.draft_probs(0).view(np.uint32), below.view(np.uint32))
        with pytest.raises(hip.Gl3Error) as ei:
            t.draft_probs(slot0 + k)
        assert ei.value.code == hip.E_STATE
    # the chain's last row may be put again by hand: the plan says it sampled categorically, as after the single calls
    targets[1].draft_probs_put(slot0 + k + 1, drafts[1])
    assert np.array_equal(targets[1].draft_probs(slot0 + k + 1).view(np.uint32), rows[-1].view(np.uint32))
    toks = [prompt[-1]] + want.tolist()
    vcoins = np.asarray([rng.next_float() for _ in range(2 * (k + 1))], F32).reshape(k + 1, 2)
    res = [t.forward_batch_verify_dist(toks, [0] * (k + 1), list(range(pos, pos + k + 1)), [T], vcoins, list(range(slot0, slot0 + k)) + [-1]) for t in targets]
    assert len(res[0]) == 1 and res[0].tolist() == res[1].tolist()
    for p in targets + drafts:
        p.freeTornadoExecutionPlan()


def raw_plan(hip, m, max_batch):
    """A plan that gl3_create made and gl3_finalize has not seen"""
    c = m.cfg
    d = hip.ModelDesc(C.sizeof(hip.ModelDesc), c.arch, c.dim, c.hidden, c.n_layers, c.n_heads, c.n_kv_heads, c.head_size, c.vocab, c.ctx,
                      c.rms_eps, m.wtype, max_batch, 0, 0, 1, 0, 1, 1.0, 0.0, 1.0, 1.0, 0, 0, 0)
    raw = C.c_void_p()
    hip.check(hip.lib().gl3_create(C.byref(d), C.byref(raw)))
    return raw


def test_refusals(pkg, planmod):
    """Every code gl3_forward_decode_chain's header lists, each before anything is uploaded or enqueued: after every refused call a K / V row,
    the probabilities row and the target's table are what they were.  (Plans on different devices need two devices: that refusal cannot be
    exercised on one and is not exercised here.)"""
    plan_mod, hip = planmod
    L = hip.lib()
    cfg = pkg.synth.CONFIGS["tiny-llama"]
    m = pkg.synth.make_numpy(cfg, seed=81)
    V, ctx = cfg.vocab, cfg.ctx
    plan = plan_mod.HipMasterPlan(m)
    target = plan_mod.HipMasterPlan(m, prefill_batch_size=8)
    single = plan_mod.HipMasterPlan(m)                                   # max_batch <= 1: no draft table
    other_vocab = plan_mod.HipMasterPlan(pkg.synth.make_numpy(dataclasses.replace(cfg, vocab=1008), seed=82), prefill_batch_size=8)
    prompt = np.random.default_rng(83).integers(0, V, 6).tolist()
    plan.prefill(prompt, 0)
    plan.forward_decode_sample(prompt[-1], 5, 0.8, 0.0, 0.25)
    q = np.random.default_rng(84).random(V).astype(F32)
    target.draft_probs_put_host(2, q)
    good = np.full(4, 0.5, F32)
    out = np.zeros(hip.CHAIN_MAX + 1, np.int32)

    def state():
        return [np.concatenate(plan.kv(l, p)) for l in range(cfg.n_layers) for p in (0, 5, 6)] + [plan.sample_probs(), plan.x(), target.draft_probs(2)]

    def call(c, token, pos, k, T, coins, tgt, slot0, res=out):
        co = np.ascontiguousarray(coins, F32) if coins is not None else None
        return L.gl3_forward_decode_chain(c, token, pos, k, T, co.ctypes.data_as(C.c_void_p) if co is not None else None, tgt, slot0,
                                          res.ctypes.data_as(C.c_void_p) if res is not None else None)
    before = state()
    assert not before[2].any()                                           # position 6 has not been written: a refused chain must not write it
    P, T_ = plan._ctx, target._ctx
    arg = [(None, 3, 6, 2, 0.0, None, None, 0),                          # null ctx
           (P, 3, 6, 0, 0.0, None, None, 0), (P, 3, 6, -1, 0.0, None, None, 0), (P, 3, 0, hip.CHAIN_MAX + 1, 0.0, None, None, 0),      # k
           (P, -1, 6, 2, 0.0, None, None, 0), (P, V, 6, 2, 0.0, None, None, 0),                                                         # token
           (P, 3, -1, 2, 0.0, None, None, 0), (P, 3, ctx - 1, 2, 0.0, None, None, 0), (P, 3, ctx, 1, 0.0, None, None, 0),              # position
           (P, 3, 6, 2, -0.5, good, None, 0), (P, 3, 6, 2, float("nan"), good, None, 0),                                                # temperature
           (P, 3, 6, 2, 0.8, None, None, 0), (P, 3, 6, 2, 0.8, [0.5, 1.0], None, 0), (P, 3, 6, 2, 0.8, [-0.1, 0.5], None, 0),           # coins
           (P, 3, 6, 2, 0.8, [0.5, float("nan")], None, 0),
           (P, 3, 6, 2, 0.8, good, P, 0),                                                                                              # target == ctx
           (P, 3, 6, 2, 0.8, good, T_, -1), (P, 3, 6, 2, 0.8, good, T_, 7), (P, 3, 6, 4, 0.8, good, T_, 5),                             # slots
           (P, 3, 6, 2, 0.8, good, other_vocab._ctx, 0)]                                                                               # vocabularies
    for a in arg:
        assert call(*a) == hip.E_ARG, a
        assert a[0] is None or L.gl3_last_error(a[0]), a
    assert call(P, 3, 6, 2, 0.0, None, None, 0, res=None) == hip.E_ARG    # null tokens_out
    assert call(P, 3, 6, 2, 0.0, None, T_, 0) == hip.E_STATE              # a greedy chain has no rows for a target
    assert call(P, 3, 6, 2, 0.8, good, single._ctx, 0) == hip.E_UNSUPPORTED
    for mb, tgt_of in ((1, None), (8, "target")):                        # before gl3_finalize: the chaining plan, then the target
        raw = raw_plan(hip, m, mb)
        try:
            code = call(P, 3, 6, 2, 0.8, good, raw, 0) if tgt_of else call(raw, 3, 6, 2, 0.0, None, None, 0)
            assert code == hip.E_STATE, (mb, code)
        finally:
            L.gl3_destroy(raw)
    with pytest.raises(hip.Gl3Error) as ei:
        plan.forward_decode_chain(3, 6, 2, 0.8, None)
    assert ei.value.code == hip.E_ARG
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(before, state()))
    for s in (0, 1, 3):
        with pytest.raises(hip.Gl3Error) as ei:
            target.draft_probs(s)
        assert ei.value.code == hip.E_STATE
    # the edges that are valid: the last positions of the context, the last slots of the table, coins unused by a greedy chain
    assert len(plan.forward_decode_chain(3, ctx - 2, 2, 0.8, good[:2], target, 6)) == 2
    assert len(plan.forward_decode_chain(3, ctx - 1, 1, 0.0, None)) == 1
    for p in (plan, target, single, other_vocab):
        p.freeTornadoExecutionPlan()


def test_tensor_parallel_plans_are_refused(pkg, orc, planmod):
    """tp_size > 1 (two ranks as threads on one GPU): GL3_E_UNSUPPORTED on every rank as the chaining plan and as the target of a one-rank
    plan's chain, and nothing is enqueued — the static-batched decode step that follows on both ranks equals the oracle bit for bit."""
    plan_mod, hip = planmod
    tp, nseq = 2, 3
    cfg = pkg.synth.CONFIGS["tiny-llama"]
    m = pkg.synth.make_numpy(cfg, seed=85)
    toks = np.random.default_rng(86).integers(0, cfg.vocab, nseq).tolist()
    ref = [orc.COracle(m).forward(t, 0) for t in toks]
    one_rank = plan_mod.HipMasterPlan(m)
    one_rank.forward_decode_sample(3, 0, 0.9, 0.0, 0.5)
    row = one_rank.sample_probs()
    grp = plan_mod.make_local_group(tp)
    out, err = [None] * tp, [None] * tp
    co = np.full(2, 0.5, F32)
    sync = threading.Barrier(tp)
    lock = threading.Lock()

    def rank_main(r):
        try:
            plan = plan_mod.HipMasterPlan(m, prefill_batch_size=8, n_seqs=nseq, tp_rank=r, tp_size=tp, local_group=grp)
            calls = [lambda: plan.forward_decode_chain(3, 0, 2, 0.0), lambda: plan.forward_decode_chain(3, 0, 2, 0.8, co),
                     lambda: one_rank.forward_decode_chain(3, 1, 2, 0.8, co, plan, 0)]
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
                assert np.array_equal(one_rank.sample_probs().view(np.uint32), row.view(np.uint32)) and not one_rank.kv(0, 1)[0].any()
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
        assert codes == [hip.E_UNSUPPORTED] * 3, (r, codes)
        for s in range(nseq):
            assert np.array_equal(logits[s], ref[s]), (r, s)
            assert int(ids[s]) == orc.argmax(ref[s])


def test_a_chain_of_chain_max(pkg, planmod):
    """One chain of GL3_CHAIN_MAX steps fills the device lists to their last entry; greedy and sampled, the ids are the single calls'."""
    plan_mod, hip = planmod
    k = hip.CHAIN_MAX
    cfg = dataclasses.replace(pkg.synth.CONFIGS["tiny-llama"], ctx=2 * k + 4)
    m = pkg.synth.make_numpy(cfg, seed=87)
    one, chain = plan_mod.HipMasterPlan(m), plan_mod.HipMasterPlan(m)
    rng = pkg.javarand.L32X64MixRandom(11)
    token = 5
    for T, pos in ((0.8, 0), (0.0, k)):
        token = run_pair(pkg, one, chain, cfg, token, pos, k, T, rng, ("chain max", T))
    for p in (one, chain):
        p.freeTornadoExecutionPlan()
