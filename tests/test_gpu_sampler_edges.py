"""The device sampler (csrc/gl3_sample.hip) on the crafted rows of tests/sampler_cases.py: vocabulary, candidate-count and cdf edges that
logits out of random-weight models reach only by chance.  tests/test_sampler_cases.py proves on the oracle alone that every case crosses
the boundary its tag names; here the same table goes through gl3_sample_rows (calls of 1, 3 and 8 rows, greedy, categorical and top-p
rows mixed, every row count many times over so all but its first call replay a graph; once more launch by launch) and the short
vocabularies through gl3_forward_decode_sample (256 workgroups per element-wise launch on rows of 16 elements).

No tolerance anywhere: ids equal orc.sample's (the reference's heap) or orc.argmax's, probabilities equal the oracle's bit for bit
(subnormals and zeros included), the logits come back untouched, and per call gl3_get_topp_counts moves by exactly (top-p rows the device
answers, top-p rows it hands to the host heap) as the sorted restatement predicts: the host gets a row whose sampled rank is tied or whose
cumulative sum reaches the three candidates the reference's heap does not emit in sorted order (sampler_cases.sorted_prefix), no other."""
import dataclasses

import numpy as np
import pytest

import __graft_entry__ as ge
import sampler_cases as sc

pytestmark = pytest.mark.gpu
MAX_BATCH = 8
CALL_SIZES = (1, 3, 8)


@pytest.fixture(scope="module")
def planmod():
    from importlib import import_module
    ge.load_package()
    return import_module(ge.PKG_NAME + ".plan"), import_module(ge.PKG_NAME + ".hip")


def model_of(pkg, V):
    return pkg.synth.make_numpy(dataclasses.replace(pkg.synth.CONFIGS["tiny-llama"], vocab=V), seed=5)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def calls_of(cases, seed):
    """The cases in a shuffled order (so the kinds mix), cut into calls of 1, 3, 8, 1, 3, 8, .. rows; a call of 3 or 8 rows holds one greedy
    row, on the logits of one of its cases, at a position that moves from call to call.  -> [[(case, greedy)]]"""
    order = np.random.default_rng(seed).permutation(len(cases))
    out, i, k = [], 0, 0
    while i < len(order):
        n = CALL_SIZES[k % 3]
        take = [cases[j] for j in order[i:i + max(n - 1, 1)]]
        i += len(take)
        rows = [(c, False) for c in take]
        if n > 1:
            rows.insert(k % (len(rows) + 1), (take[k % len(take)], True))
        out.append(rows)
        k += 1
    return out


def run_calls(plan, orc, calls):
    """every call through sample_rows against the oracle; returns (top-p rows the device answered, rows the host heap answered)"""
    total = [0, 0]
    for rows in calls:
        logits = np.stack([c.logits for c, _ in rows])
        keep = logits.copy()
        temps = [0.0 if greedy else c.temperature for c, greedy in rows]
        topps = [c.topp for c, _ in rows]
        coins = [0.0 if greedy else c.coin for c, greedy in rows]
        before = plan.topp_counts()
        ids = plan.sample_rows(logits, temps, topps, coins)
        after = plan.topp_counts()
        assert ids.dtype == np.int32 and ids.shape == (len(rows),)
        assert same_bits(logits, keep)
        device = host = 0
        for i, (c, greedy) in enumerate(rows):
            if greedy:
                assert ids[i] == orc.argmax(c.logits), (c.tag, "greedy")
                continue
            want, probs = orc.sample(c.logits, c.temperature, c.topp, c.coin, want_probs=True)
            assert same_bits(plan.sample_probs_row(i), probs), (c.tag, len(rows), i)
            assert ids[i] == want, (c.tag, len(rows), i, int(ids[i]), want)
            if sc.is_topp(c.temperature, c.topp):
                to_host = sc.sorted_topp(probs, c.topp, c.coin).host
                host += to_host
                device += not to_host
        assert (after[0] - before[0], after[1] - before[1]) == (device, host), [c.tag for c, _ in rows]
        total[0] += device
        total[1] += host
    return tuple(total)


@pytest.mark.parametrize("V", sc.VOCABS)
def test_the_case_table_through_sample_rows(pkg, orc, planmod, V):
    plan_mod, _ = planmod
    plan = plan_mod.HipMasterPlan(model_of(pkg, V), prefill_batch_size=MAX_BATCH)
    calls = calls_of(sc.cases(V), V)
    assert {len(rows) for rows in calls} >= ({1, 3, 8}) and sum(len(rows) for rows in calls) >= len(sc.cases(V))
    device, host = run_calls(plan, orc, calls)
    assert device > 0 and host > 0
    plan.freeTornadoExecutionPlan()


def test_the_case_table_launch_by_launch(pkg, orc, planmod):
    """V = 4112 (a second chunk and a last sort tile of 16 elements) with graphs off: the same launches, enqueued one by one"""
    plan_mod, hip = planmod
    V = 4112
    plan = plan_mod.HipMasterPlan(model_of(pkg, V), prefill_batch_size=MAX_BATCH, flags=hip.FLAG_NO_GRAPH)
    run_calls(plan, orc, calls_of(sc.cases(V), V + 1))
    plan.freeTornadoExecutionPlan()


@pytest.mark.parametrize("V", sc.VOCABS)
def test_sort_stability(pkg, orc, planmod, V):
    """V - 1 equal candidates and one larger value in the middle of the row: four stable passes over equal keys must bring it to rank 0
    and leave the rest in index order.  Coins on rank 0 (its lowest and its highest) are answered by the device, with that index and no
    host flag; the coin on rank 1, a tied rank, by the host."""
    plan_mod, _ = planmod
    plan = plan_mod.HipMasterPlan(model_of(pkg, V), prefill_batch_size=MAX_BATCH)
    rows = sc.stability_cases(V)
    j = int(np.argmax(rows[0].logits))
    before = plan.topp_counts()
    ids = plan.sample_rows(np.stack([c.logits for c in rows]), [c.temperature for c in rows], [c.topp for c in rows], [c.coin for c in rows])
    after = plan.topp_counts()
    assert ids[0] == j and ids[1] == j
    assert ids.tolist() == [orc.sample(c.logits, c.temperature, c.topp, c.coin) for c in rows]
    assert (after[0] - before[0], after[1] - before[1]) == (2, 1)
    plan.freeTornadoExecutionPlan()


SINGLE = [(1.0, 0.0), (0.7, 0.95), (0.02, 0.9), (5.0, 0.0), (1.3, 0.5), (0.4, 1.0)]      # (temperature, topp): categorical and top-p in turn


@pytest.mark.parametrize("V", sc.VOCABS)
def test_single_row_entry(pkg, orc, planmod, V):
    """gl3_forward_decode_sample launches 256 workgroups per element-wise kernel whatever the vocabulary: at V = 16 all but one of them
    have no element and contribute a block maximum of -inf; at V = 1008 most lanes of every workgroup are idle.  6 decode steps against
    COracle, Java-generator coins, ids and sample_probs() bit for bit, the top-p draws counted where the restatement says."""
    plan_mod, _ = planmod
    m = model_of(pkg, V)
    plan = plan_mod.HipMasterPlan(m)
    o = orc.COracle(m)
    rng = pkg.javarand.L32X64MixRandom(1234)
    tok, device, host = 1, 0, 0
    for pos, (temperature, topp) in enumerate(SINGLE):
        coin = rng.next_float()
        want, probs = orc.sample(o.forward(tok, pos), temperature, topp, coin, want_probs=True)
        got = plan.forward_decode_sample(tok, pos, temperature, topp, coin)
        assert same_bits(plan.sample_probs(), probs), (V, pos)
        assert got == want, (V, pos, temperature, topp, coin)
        if sc.is_topp(temperature, topp):
            to_host = sc.sorted_topp(probs, topp, coin).host
            host += to_host
            device += not to_host
        tok = got
    assert plan.topp_counts() == (device, host)
    plan.freeTornadoExecutionPlan()
