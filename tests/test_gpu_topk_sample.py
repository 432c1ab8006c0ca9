"""The top-k / min-p / top-p sampler (csrc/gl3_topk_sample.h) against the NumPy restatement of its contract (tests/topk_ref.py): ids, kk,
n_keep and the tap's survivor ids exactly equal, the tap's probabilities bit for bit.  Crafted rows through gl3_sample_rows_topk on
vocabularies off the kernel's granularities: 1008 (below 1024, one iteration per wavefront slab), 5040 (slabs of 79 quads, no multiple of
the 64-quad iteration; pass 0 never takes its lower bound) and 12304 (16 above 3 * 4096: the lower-bound path, a shorter last slab).
gl3_create admits only multiples of 16, so no vocabulary that is not a multiple of 4 can be built.  Then the two model entries and
tools/gl3_run --top-k on java.util.Random coins."""
import dataclasses
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import topk_ref as ref

pytestmark = pytest.mark.gpu
F32 = np.float32
VOCABS = (1008, 5040, 12304)
TOP_KS = (1, 2, 40, 1024)
COINS = (0.0, 0.5, float(np.nextafter(F32(1), F32(0))))
KINDS = ("generic", "equal", "tie-block", "one-binade", "zeros", "ninf-few", "ninf-many", "dominant")
MAX_BATCH = 96
RUN = os.path.join(ge.ROOT, "tools", "gl3_run")


@pytest.fixture(scope="module")
def mods(pkg):
    from importlib import import_module
    return import_module(ge.PKG_NAME + ".plan"), import_module(ge.PKG_NAME + ".hip")


@pytest.fixture(scope="module")
def plans(pkg, mods):
    made = {}

    def get(V):
        if V not in made:
            made[V] = mods[0].HipMasterPlan(pkg.synth.make_numpy(dataclasses.replace(pkg.synth.CONFIGS["tiny-llama"], vocab=V), seed=5), prefill_batch_size=MAX_BATCH)
        return made[V]
    yield get
    for p in made.values():
        p.freeTornadoExecutionPlan()


def crafted(kind, V):
    rng = np.random.default_rng(V + len(kind))
    lg = (rng.standard_normal(V) * 2.0).astype(F32)
    if kind == "equal":                      # index order decides everything
        lg[:] = F32(0.25)
    elif kind == "tie-block":                # one maximum, then equal values over ranks 1 .. 1100 (V = 1008: 600): every top_k > 1 ends inside them
        block = rng.permutation(V)[:min(1100, 600 if V < 1100 else V)]
        lg[block] = F32(7.0)
        lg[block[0]] = F32(8.0)
    elif kind == "one-binade":               # 1.0f + i * 2^-23: the whole row in one top-digit bucket, and in one bucket of the second pass per 1024
        lg = (F32(1.0) + np.arange(V, dtype=F32) * F32(2.0 ** -23)).astype(F32)
        return lg, 1e-5
    elif kind == "zeros":                    # 20 positive logits, 200 zeros of both signs in turn, the rest negative: top_k = 40 ends among the zeros
        lg = -np.abs(lg) - F32(0.5)
        idx = rng.permutation(V)
        lg[idx[:20]] = np.abs(lg[idx[:20]])
        lg[idx[20:220:2]], lg[idx[21:220:2]] = F32(0.0), F32(-0.0)
    elif kind == "ninf-few":                 # fewer than vocab - k
        lg[rng.permutation(V)[:V // 4]] = -np.inf
    elif kind == "ninf-many":                # 30 finite logits: top_k = 40 takes the ten -inf of lowest index
        keep = lg[:30].copy()
        lg[:] = -np.inf
        lg[rng.permutation(V)[:30]] = keep
    elif kind == "dominant":                 # n_keep == 1 under either cut
        lg[V // 3] = F32(60.0)
    return lg, 0.8


def aimed_cuts(kind, lg, k, T):
    """(minp, topp) pairs: off, each cutting inside the survivors (aimed at their middle), each cutting nothing, both, both out of range"""
    if kind == "dominant":                   # the second probability is ~1e-29: any ordinary cut keeps one entry
        return ((0.0, 0.0), (0.05, 0.0), (0.0, 0.9), (0.05, 0.9))
    p = ref.sample(lg, k, T, 0.0, 0.0, 0.0)[2]
    h = p.size // 2
    minp_in = float(min(F32(1), np.nextafter(F32(p[h] / p[0]), F32(2))))
    topp_in = float(np.cumsum(p, dtype=F32)[max(h - 1, 0)]) if p.size > 1 else 0.5
    return ((0.0, 0.0), (minp_in, 0.0), (1e-30, 0.0), (0.0, topp_in), (0.0, COINS[2]), (minp_in, topp_in), (2.0, 1.0))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("V", VOCABS)
def test_crafted_rows(plans, mods, V, kind):
    plan, hip = plans(V), mods[1]
    lg, T = crafted(kind, V)
    rows = [(k, T, topp, minp, coin) for k in TOP_KS for minp, topp in aimed_cuts(kind, lg, k, T) for coin in COINS]
    rows.insert(5, (0, 0.0, 0.0, 0.0, 0.0))             # greedy rows: their other settings are not looked at
    rows.append((5000, 0.0, 7.0, -1.0, 9.0))
    got = plan.sample_rows_topk(np.tile(lg, (len(rows), 1)), *[list(c) for c in zip(*rows)])
    for i, (k, temperature, topp, minp, coin) in enumerate(rows):
        if temperature == 0.0:
            assert got[i] == int(np.argmax(lg)), (i, "greedy")
            with pytest.raises(hip.Gl3Error) as e:
                plan.topk_row(i)
            assert e.value.code == hip.E_STATE
            continue
        token, ids, p, n_keep = ref.sample(lg, k, temperature, topp, minp, coin)
        t_ids, t_p, t_keep = plan.topk_row(i)
        assert t_ids.size == min(k, V) and np.array_equal(t_ids, ids), (i, rows[i])
        assert np.array_equal(t_p, p), (i, rows[i])
        assert t_keep == n_keep and got[i] == token, (i, rows[i], t_keep, n_keep, int(got[i]), token)
        if kind == "dominant" and (minp or topp):
            assert n_keep == 1


def test_refusals(pkg, plans, mods):
    plan_mod, hip = mods
    V = VOCABS[0]
    lg = np.zeros((1, V), F32)
    for k in (0, 1025):
        with pytest.raises(hip.Gl3Error) as e:
            plans(V).sample_rows_topk(lg, k, 0.8, 0.9, 0.05, 0.5)
        assert e.value.code == hip.E_ARG
    single = plan_mod.HipMasterPlan(pkg.synth.make_numpy(pkg.synth.CONFIGS["tiny-llama"], seed=5))
    with pytest.raises(hip.Gl3Error) as e:
        single.sample_rows_topk(np.zeros((1, single.cfg.vocab), F32), 40, 0.8, 0.9, 0.05, 0.5)
    assert e.value.code == hip.E_UNSUPPORTED
    single.freeTornadoExecutionPlan()


def test_model_entries(pkg, orc, mods, tmp_path):
    """gl3_forward_batch_sample_topk and gl3_forward_decode_sample_topk return the restatement's ids on the logits of gl3_forward_batch /
    gl3_forward_decode; tools/gl3_run --top-k prints the restatement's ids over the oracle's logits, java.util.Random coins, twice."""
    m = pkg.synth.make_numpy(pkg.synth.CONFIGS["tiny-llama"], seed=11)
    settings = [(40, 0.8, 0.95, 0.05, 0.3), (0, 0.0, 0.0, 0.0, 0.0), (3, 1.2, 0.0, 0.0, 0.9), (1024, 0.7, 0.9, 0.0, 0.6)]
    plan = mods[0].HipMasterPlan(m, prefill_batch_size=4, n_seqs=4)
    toks, seqs, pos = [5, 9, 17, 33], [0, 1, 2, 3], [0, 0, 0, 0]
    logits, greedy = plan.forward_batch(toks, seqs, pos)
    got = plan.forward_batch_sample_topk(toks, seqs, pos, *[list(c) for c in zip(*settings)])
    want = [int(greedy[i]) if s[1] == 0.0 else ref.sample(logits[i], *s)[0] for i, s in enumerate(settings)]
    assert got.tolist() == want
    assert plan.topk_row(3)[2] == ref.sample(logits[3], *settings[3])[3]
    plan.freeTornadoExecutionPlan()
    plan = mods[0].HipMasterPlan(m)
    tok = 7
    for position, s in enumerate(settings):
        lg = plan.forward_decode(tok, position)
        nxt = plan.forward_decode_sample_topk(tok, position, *s)
        assert nxt == (int(np.argmax(lg)) if s[1] == 0.0 else ref.sample(lg, *s)[0]), position
        tok = nxt
    plan.freeTornadoExecutionPlan()

    path = str(tmp_path / "m.gguf")
    m.write_gguf(path)
    prompt = pkg.javarand.bench_tokens(m.cfg.vocab, 5)
    o, rng = orc.COracle(pkg.synth.SynthModel.from_gguf(path)), pkg.javarand.JavaRandom(77)
    want, cur = [], 1
    for position in range(20):               # generateTokensGPULlama: begin-of-text, the prompt, then the sampled ids
        lg = o.forward(cur, position)
        cur = prompt[position] if position < len(prompt) else ref.sample(lg, 40, 0.8, 0.95, 0.05, F32(rng.next(24)) / F32(1 << 24))[0]
        want += [cur] if position >= len(prompt) else []
    cmd = [RUN, "-m", path, "--ids", ",".join(map(str, prompt)), "-n", "20", "--bos", "1", "--top-k", "40", "--min-p", "0.05", "--top-p", "0.95",
           "--temperature", "0.8", "--seed", "77", "--rng", "lcg"]
    for _ in range(2):
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=180)
        assert out.returncode == 0, out.stderr
        assert [int(x) for x in out.stdout.split("generated:")[1].split()] == want
