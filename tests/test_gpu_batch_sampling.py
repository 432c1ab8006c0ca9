"""gl3_forward_decode_batch_sample / gl3_sample_rows on the GPU against the oracle's Sampler.selectSampler restatement, row by row:
the same sampled id for the same rng.nextFloat(1f) and the same probabilities bit for bit (np.array_equal, no tolerance), with
greedy, categorical and top-p rows sharing one step, for every weight class that has static-batched decode."""
import numpy as np
import pytest

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu

# (temperature, topp): greedy, categorical (topp outside (0, 1)) and top-p rows
SETTINGS = [(0.7, .95), (1.0, 0), (0, .9), (0.4, .5), (1.3, 1.0), (0.1, .95), (0.02, .9), (3.0, .999)]
DRAWS = {"device": 0, "host": 0}            # top-p draws of tests 1-3, for the device-share check at the end of the file


@pytest.fixture(scope="module")
def planmod():
    from importlib import import_module
    ge.load_package()
    return import_module(ge.PKG_NAME + ".plan"), import_module(ge.PKG_NAME + ".hip")


def is_topp(temperature, topp):
    return temperature > 0 and 0 < topp < 1


def count_draws(plan):
    dev, host = plan.topp_counts()
    DRAWS["device"] += dev
    DRAWS["host"] += host
    return dev, host


def mixed_generation(pkg, orc, plan, oracles, m, nseq, steps, lens=None):
    """prefill nseq prompts of different lengths (lens; default 3, 5, 7, ..), then `steps` batched sampled steps; row order reversed on odd
    steps; row s at step t uses SETTINGS[(s + t) % 8]; coins from one L32X64MixRandom(1234) in (step, sequence) order, non-greedy rows only."""
    rng = np.random.default_rng(3)
    lens = list(lens) if lens is not None else [3 + 2 * i for i in range(nseq)]
    assert len(lens) == nseq
    prompts = [rng.integers(0, m.cfg.vocab, n).tolist() for n in lens]
    for s in range(nseq):
        plan.prefill_seq(s, prompts[s], 0)
        oracles[s].prefill(prompts[s], 0)
    cur = [int(rng.integers(0, m.cfg.vocab)) for _ in range(nseq)]
    pos = list(lens)
    jr = pkg.javarand.L32X64MixRandom(1234)
    n_topp = 0
    for step in range(steps):
        sets = [SETTINGS[(s + step) % 8] for s in range(nseq)]
        coins = [jr.next_float() if sets[s][0] > 0 else 0.0 for s in range(nseq)]
        order = list(range(nseq))
        if step % 2:
            order.reverse()
        ids = plan.forward_decode_batch_sample([cur[s] for s in order], order, [pos[s] for s in order], [sets[s][0] for s in order],
                                               [sets[s][1] for s in order], [coins[s] for s in order])
        assert ids.dtype == np.int32 and ids.shape == (nseq,)
        for row, s in enumerate(order):
            temperature, topp = sets[s]
            logits = oracles[s].forward(cur[s], pos[s])
            if temperature > 0:
                want, probs = orc.sample(logits, temperature, topp, coins[s], want_probs=True)
                assert np.array_equal(plan.sample_probs_row(row), probs), (step, s, temperature, topp)
                n_topp += is_topp(temperature, topp)
            else:
                want = orc.argmax(logits)
            assert ids[row] == want, (step, s, temperature, topp, coins[s])
            cur[s], pos[s] = int(ids[row]), pos[s] + 1          # every sequence continues with its own sampled token
    return cur, pos, n_topp


@pytest.mark.parametrize("cfg", ["mid-llama", "tiny-qwen3"])
def test_batched_generation_with_mixed_settings(pkg, orc, planmod, cfg):
    plan_mod, hip = planmod
    nseq = 8
    m = pkg.synth.make_numpy(pkg.synth.CONFIGS[cfg], seed=83)
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=16, n_seqs=nseq)
    oracles = [orc.COracle(m) for _ in range(nseq)]
    cur, pos, n_topp = mixed_generation(pkg, orc, plan, oracles, m, nseq, 6)
    dev, host = count_draws(plan)
    assert n_topp == 30 and dev + host == n_topp, (dev, host)
    # every temperature 0: the ids of the greedy batched step (a coin of 1.0 on a greedy row is not looked at)
    order = list(range(nseq))
    got = plan.forward_decode_batch_sample(cur, order, pos, 0.0, 0.9, 1.0)
    want = plan.forward_decode_batch(cur, order, pos, want_logits=False)[1]
    assert np.array_equal(got, want)
    for s in range(nseq):
        assert got[s] == orc.argmax(oracles[s].forward(cur[s], pos[s]))
    with pytest.raises(hip.Gl3Error):
        plan.sample_probs_row(0)                               # no probabilities behind a greedy step
    assert plan.topp_counts() == (dev, host)
    plan.freeTornadoExecutionPlan()


@pytest.mark.parametrize("wtype", [1, 2])      # F16, Q4_0: the Vector-API-order GEMMs feed the same sampler
def test_batched_sampling_of_the_f32_activation_weight_classes(pkg, orc, planmod, wtype):
    plan_mod, hip = planmod
    nseq = 4
    m = pkg.synth.make_numpy(pkg.synth.CONFIGS["mid-llama"], wtype=wtype, seed=83)
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=16, n_seqs=nseq)
    oracles = [orc.COracle(m, vector_bits=256, f32_activation=False) for _ in range(nseq)]
    _, _, n_topp = mixed_generation(pkg, orc, plan, oracles, m, nseq, 3)
    dev, host = count_draws(plan)
    assert dev + host == n_topp and n_topp > 0, (dev, host)
    plan.freeTornadoExecutionPlan()


def test_full_vocabulary_rows_through_the_sampler_alone(pkg, orc, planmod):
    """vocab 128256 (31 exact chunks of 4096 + one of 1280 per row), 8 rows with 8 different settings in one call; coins 0.0 and
    0.999999 on the two categorical rows land in the first and the last chunk of the cdf."""
    plan_mod, hip = planmod
    import torch
    cfg = pkg.synth.CONFIGS["8b-vocab"]
    m = pkg.synth.make_torch(cfg, seed=89, device="cuda" if torch.cuda.is_available() else "cpu")
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=16, n_seqs=2)
    o = orc.COracle(m)
    tokens = [128000, 1, 777, 4095, 65536, 100000, 31337, 128255]
    logits = np.stack([o.forward(t, 0) for t in tokens])
    jr = pkg.javarand.L32X64MixRandom(1234)
    coins = [jr.next_float() if SETTINGS[i][0] > 0 else 0.0 for i in range(8)]
    coins[1], coins[4] = 0.0, 0.999999
    ids = plan.sample_rows(logits, [s[0] for s in SETTINGS], [s[1] for s in SETTINGS], coins)
    for i, (temperature, topp) in enumerate(SETTINGS):
        if temperature > 0:
            want, probs = orc.sample(logits[i], temperature, topp, coins[i], want_probs=True)
            assert np.array_equal(plan.sample_probs_row(i), probs), (i, temperature, topp)
        else:
            want = orc.argmax(logits[i])
            with pytest.raises(hip.Gl3Error):
                plan.sample_probs_row(i)
        assert ids[i] == want, (i, temperature, topp, coins[i])
    dev, host = count_draws(plan)
    assert dev + host == 5, (dev, host)
    plan.freeTornadoExecutionPlan()


def tied_at_the_sampled_rank(probs, topp, token):
    """how many top-p candidates (ToppSampler.java:73-81) share the sampled token's probability"""
    cutoff = np.float32(np.float32(1.0) - np.float32(topp)) / np.float32(probs.size - 1)
    return int(np.count_nonzero(probs[probs >= cutoff] == probs[token]))


def test_ties_go_to_the_host_heap_row_by_row(pkg, orc, planmod):
    plan_mod, hip = planmod
    m = pkg.synth.make_numpy(pkg.synth.CONFIGS["mid-llama"], seed=83)
    assert m.cfg.vocab == 4096
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=16, n_seqs=2)
    o = orc.COracle(m)
    logits = np.empty((6, 4096), np.float32)
    for row in range(6):
        logits[row] = 0.25 if row in (1, 4) else o.forward(100 + 37 * row, 0)      # rows 1 and 4: every candidate ties
    jr = pkg.javarand.L32X64MixRandom(1234)
    coins, want = [], []
    for row in range(6):
        while True:
            coin = jr.next_float()
            tok, probs = orc.sample(logits[row], 1.0, 0.9, coin, want_probs=True)
            ties = tied_at_the_sampled_rank(probs, 0.9, tok)
            if row in (1, 4):
                assert ties == 4096
                break
            if ties == 1:                                       # a model row must be tie-free for the exact (+4, +2) below
                break
        coins.append(coin); want.append(tok)
    dev0, host0 = plan.topp_counts()
    ids = plan.sample_rows(logits, 1.0, 0.9, coins)
    assert ids.tolist() == want
    dev1, host1 = plan.topp_counts()
    assert (dev1 - dev0, host1 - host0) == (4, 2)
    plan.freeTornadoExecutionPlan()


def oracle_ties(pkg, orc, m, nseq, steps):
    """the settings and coin stream of test 1 on the oracle alone, decode from position 0: (top-p draws, ties at the sampled rank)"""
    oracles = [orc.COracle(m) for _ in range(nseq)]
    jr = pkg.javarand.L32X64MixRandom(1234)
    cur, draws, ties = [1 + s for s in range(nseq)], 0, 0
    for step in range(steps):
        for s in range(nseq):
            temperature, topp = SETTINGS[(s + step) % 8]
            logits = oracles[s].forward(cur[s], step)
            if temperature == 0:
                cur[s] = orc.argmax(logits)
                continue
            tok, probs = orc.sample(logits, temperature, topp, jr.next_float(), want_probs=True)
            if is_topp(temperature, topp):
                draws += 1
                ties += tied_at_the_sampled_rank(probs, topp, tok) > 1
            cur[s] = tok
    return draws, ties


def test_device_share_of_the_top_p_draws(pkg, orc, planmod):
    """Host fallbacks (a tie at the sampled rank) are at most 20 % of the top-p draws, the cap tests/test_gpu_sampling.py uses: on the
    oracle alone for the models and the coin stream of the tests above, and over the draws those tests counted on the device."""
    import torch
    for cfg in ("mid-llama", "tiny-qwen3", "tiny-llama"):
        draws, ties = oracle_ties(pkg, orc, pkg.synth.make_numpy(pkg.synth.CONFIGS[cfg], seed=83), 8, 6)
        print(cfg, "top-p draws", draws, "ties at the sampled rank", ties)
        assert draws == 30 and ties <= 0.2 * draws, (cfg, draws, ties)
    m = pkg.synth.make_torch(pkg.synth.CONFIGS["8b-vocab"], seed=89, device="cuda" if torch.cuda.is_available() else "cpu")
    draws, ties = oracle_ties(pkg, orc, m, 8, 3)
    print("8b-vocab top-p draws", draws, "ties at the sampled rank", ties)
    assert draws == 15 and ties <= 0.2 * draws, (draws, ties)
    print("device", DRAWS)
    total = DRAWS["device"] + DRAWS["host"]
    assert DRAWS["host"] <= 0.2 * total, DRAWS


def test_argument_errors(pkg, orc, planmod):
    plan_mod, hip = planmod
    m = pkg.synth.make_numpy(pkg.synth.CONFIGS["tiny-qwen3"], seed=83)
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=4, n_seqs=8)
    o = orc.COracle(m)
    with pytest.raises(hip.Gl3Error):
        plan.sample_probs_row(0)                                                       # before any sampled step
    with pytest.raises(hip.Gl3Error):
        plan.forward_decode_batch_sample([1, 2], [0, 1], [0, 0], [0.7, 0.0], 0.9, [1.0, 0.5])       # coin must be < 1 on a non-greedy row
    with pytest.raises(hip.Gl3Error):
        plan.forward_decode_batch_sample([1, 2], [0, 1], [0, 0], [0.7, float("nan")], 0.9, 0.5)
    with pytest.raises(hip.Gl3Error):
        plan.forward_decode_batch_sample([1] * 5, list(range(5)), [0] * 5, 0.7, 0.9, 0.5)           # n > max_batch
    with pytest.raises(hip.Gl3Error):
        plan.sample_rows(np.zeros((5, m.cfg.vocab), np.float32), 0.7, 0.9, 0.5)
    with pytest.raises(hip.Gl3Error):
        plan.forward_decode_batch_sample([1, 2], [0, 0], [0, 0], 0.7, 0.9, 0.5)                     # duplicate sequence id
    # a coin of 1.0 on a greedy row is ignored
    ids = plan.forward_decode_batch_sample([1, 2], [0, 1], [0, 0], [0.0, 0.7], 0.9, [1.0, 0.25])
    l0, l1 = o.forward(1, 0), orc.COracle(m).forward(2, 0)
    assert ids[0] == orc.argmax(l0) and ids[1] == orc.sample(l1, 0.7, 0.9, 0.25)
    single = plan_mod.HipMasterPlan(m)                                                 # max_batch <= 1: no batched decode, no batched sampler
    with pytest.raises(hip.Gl3Error) as e:
        single.sample_rows(np.zeros((1, m.cfg.vocab), np.float32), 0.7, 0.9, 0.5)
    assert e.value.code == hip.E_UNSUPPORTED
    single.freeTornadoExecutionPlan()
    plan.freeTornadoExecutionPlan()
