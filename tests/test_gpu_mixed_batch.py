"""The mixed batched step (gl3_forward_batch / gl3_forward_batch_sample): prompt chunks and decode rows of many sequences in one pass,
bit for bit against one CPU oracle per sequence.

A row's arithmetic does not depend on which other rows share its step, so every comparison is np.array_equal on f32 against the
oracle run of that row's own sequence: logits and greedy id of every output row, x of the step's last row, and the K / V rows the
step wrote (first, middle and last of every run, every layer).  The attention of a step with a run of several rows is the run-table
form of the one-launch prefill kernels (pf_attn_fused3_kernel<64 | 128, true>, pf_attn_fused2_kernel<.., true>) or, for shapes and
depths they do not cover, the per-row pair; the logits stage runs over the flagged rows only."""
import os
import subprocess
import sys

import numpy as np
import pytest

import __graft_entry__ as ge
from test_gpu_batch_decode_depth import model_with_ctx
# test_gpu_batch_sampling.py keeps a module-global tally of top-p draws (count_draws): nothing here counts into it
from test_gpu_batch_sampling import SETTINGS, is_topp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tools", "gl3_batch_run")


@pytest.fixture(scope="module")
def planmod():
    from importlib import import_module
    ge.load_package()
    return import_module(ge.PKG_NAME + ".plan"), import_module(ge.PKG_NAME + ".hip")


def variant(pkg, cfg, seed, wtype=8, **over):
    base = pkg.synth.CONFIGS[cfg]
    return pkg.synth.make_numpy(pkg.synth.ModelConfig(**{**base.__dict__, **over}), wtype=wtype, seed=seed)


def oracle_for(orc, m, wtype):
    return orc.COracle(m, vector_bits=256) if wtype != 8 else orc.COracle(m)


def x_of_row(o, token, pos):
    """The residual stream behind the last layer for (token, pos) on oracle o: what gl3_get_x holds.  The oracle's forward() applies the
    output norm to x in place on its way to the logits, so the row runs without logits here (the same K / V row is written again by the
    forward() that follows)."""
    o.prefill([token], pos)
    return o.x().copy()


class Mixed:
    """n sequences on a plan and on one oracle each.  step(runs): one forward_batch of runs [(sequence, tokens)] at every sequence's own
    next position, checked row by row against the oracles."""

    def __init__(self, orc, plan, oracles, m, seed):
        self.orc, self.plan, self.oracles, self.m = orc, plan, oracles, m
        self.rng = np.random.default_rng(seed)
        self.pos = [0] * len(oracles)
        self.next_id = {}                        # sequence -> greedy id of its last output row

    def tokens(self, n):
        return self.rng.integers(0, self.m.cfg.vocab, n).tolist()

    def prefill(self, seq, n):
        """n prompt tokens through the existing one-sequence entry"""
        t = self.tokens(n)
        self.plan.prefill_seq(seq, t, self.pos[seq])
        self.oracles[seq].prefill(t, self.pos[seq])
        self.pos[seq] += n

    def arrays(self, runs, flag_all=()):
        toks, seqs, poss, want = [], [], [], []
        for seq, t in runs:
            toks += list(t); seqs += [seq] * len(t); poss += list(range(self.pos[seq], self.pos[seq] + len(t)))
            want += [1] * len(t) if seq in flag_all else [0] * (len(t) - 1) + [1]
        return toks, seqs, poss, want

    def step(self, runs, flag_all=(), explicit=False):
        """flag_all: sequences whose every row is an output row (the others: the run's last row).  The default flags go in as want_logits = None
        unless `explicit`."""
        m, plan = self.m, self.plan
        toks, seqs, poss, want = self.arrays(runs, flag_all)
        n = len(toks)
        logits, ids = plan.forward_batch(toks, seqs, poss, want if (flag_all or explicit) else None)
        assert logits.shape == (sum(want), m.cfg.vocab) and ids.shape == (sum(want),)
        out = 0
        for row in range(n):
            if row == n - 1:
                x_last = x_of_row(self.oracles[seqs[row]], toks[row], poss[row])
            ref = self.oracles[seqs[row]].forward(toks[row], poss[row])
            if want[row]:
                assert np.array_equal(logits[out], ref), ("logits", "row", row, "seq", seqs[row], "pos", poss[row], "rows", n)
                assert int(ids[out]) == self.orc.argmax(ref), ("id", "row", row, "seq", seqs[row], "pos", poss[row])
                self.next_id[seqs[row]] = int(ids[out])
                out += 1
        x = plan.x()
        assert np.array_equal(x, x_last), "x of the last row"
        dim = m.cfg.dim
        assert np.array_equal(plan.buffer(4, n * dim).reshape(n, dim)[n - 1], x), "the step's X rows are in step order"
        for seq, t in runs:
            p0 = self.pos[seq]
            for p in sorted({p0, p0 + len(t) // 2, p0 + len(t) - 1}):
                for l in range(m.cfg.n_layers):
                    k, v = plan.kv_seq(seq, l, p)
                    ko, vo = self.oracles[seq].kv(l, p)
                    assert np.array_equal(k, ko) and np.array_equal(v, vo), ("kv", "seq", seq, "layer", l, "pos", p)
            self.pos[seq] += len(t)


def schedule(b):
    """Step 1: two prompt runs.  Step 2: decode rows around a 17-row run whose every row is an output row (the verification use).  Step 3: a
    continuation chunk, two decode rows and a one-row run at position 0."""
    b.step([(0, b.tokens(9)), (2, b.tokens(3))])
    b.step([(0, [b.next_id[0]]), (1, b.tokens(17)), (2, [b.next_id[2]])], flag_all={1})
    b.step([(1, b.tokens(5)), (0, [b.next_id[0]]), (2, [b.next_id[2]]), (3, b.tokens(1))], explicit=True)
    assert b.pos == [11, 22, 5, 1]


SCHEDULE_CASES = [("mid-llama", 8, {}),                     # kvMul 4, head size 64: pf_attn_fused3_kernel<64, true>
                  ("mid-qwen3", 8, {"ctx": 64}),            # head size 128: fused3<128, true>, per-head norm
                  ("mid-phi3", 8, {}),                      # kvMul 3 at head size 128: no tile of 8 float4 per thread, the per-row pair
                  ("mid-qwen2", 8, {}),                     # kvMul 6: per-row pair, bias
                  ("mid-llama", 1, {}),                     # F16: pf_layers_vl
                  ("mid-qwen2moe", 8, {}),                  # grouped experts (kvMul 1 at head size 128: per-row pair)
                  ("tiny-llama", 8, {}),                    # head size 32: pf_attn_fused2_kernel<32, true>
                  ("mid-llama", 8, {"n_kv_heads": 16})]     # kvMul 2, head size 64: fused2<64, true>


@pytest.mark.parametrize("cfg,wtype,over", SCHEDULE_CASES, ids=["%s-%d%s" % (c, w, "-kv%d" % o["n_kv_heads"] if "n_kv_heads" in o else "") for c, w, o in SCHEDULE_CASES])
def test_schedule_parity(pkg, orc, planmod, cfg, wtype, over):
    plan_mod, _ = planmod
    m = variant(pkg, cfg, seed=61, wtype=wtype, **over)
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=64, n_seqs=4)
    b = Mixed(orc, plan, [oracle_for(orc, m, wtype) for _ in range(4)], m, seed=7)
    schedule(b)
    plan.freeTornadoExecutionPlan()


def test_schedule_parity_on_the_packed_f32_table_form(pkg):
    """GL3_PF_FUSED_MFMA=0 (read once per process): kvMul 4 runs pf_attn_fused2_kernel<64 | 128, true> instead of fused3."""
    e = dict(os.environ, GL3_PF_FUSED_MFMA="0")
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-k",
                          "test_schedule_parity and (mid-llama-8] or mid-qwen3-8])", "-p", "no:cacheprovider"],
                         capture_output=True, text=True, timeout=300, env=e, cwd=ROOT)
    tail = out.stdout[-1500:] + out.stderr[-500:]
    assert out.returncode == 0, tail
    assert "2 passed" in out.stdout and "failed" not in out.stdout and "skipped" not in out.stdout, tail


@pytest.mark.parametrize("cfg,ctx", [("mid-llama", 160), ("mid-qwen3", 80)])
def test_more_than_64_rows(pkg, orc, planmod, cfg, ctx):
    """93 rows, ragged against every tile size (8-row attention tiles, 16-token GEMM tiles, the 64-row threshold of the chunk-major GEMMs):
    a 70-row run, three decode rows at depths 2, 9 and 31, a 20-row run.  mid-qwen3: the attention output leaves the kernel quantised."""
    plan_mod, _ = planmod
    m = model_with_ctx(pkg, cfg, ctx, seed=63)
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=128, n_seqs=5)
    b = Mixed(orc, plan, [orc.COracle(m) for _ in range(5)], m, seed=9)
    for seq, depth in ((1, 2), (2, 9), (3, 31)):
        b.prefill(seq, depth)
    b.step([(0, b.tokens(70)), (1, b.tokens(1)), (2, b.tokens(1)), (3, b.tokens(1)), (4, b.tokens(20))])
    assert b.pos == [70, 3, 10, 32, 20]
    plan.freeTornadoExecutionPlan()


def test_depth_fallback(pkg, orc, planmod):
    """A decode row at position 560 next to a 12-row prompt run: the deepest row's score rows do not fit LDS beside the query rows, the whole
    step takes the per-row pair."""
    plan_mod, _ = planmod
    m = model_with_ctx(pkg, "mid-qwen3", 600, seed=65)
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=64, n_seqs=2)
    b = Mixed(orc, plan, [orc.COracle(m) for _ in range(2)], m, seed=11)
    b.prefill(0, 560)
    b.step([(0, b.tokens(1)), (1, b.tokens(12))])
    assert b.pos == [561, 12]
    plan.freeTornadoExecutionPlan()


def test_single_row_steps(pkg, orc, planmod):
    """Four single rows at positions 3, 127, 128 and 130 (both sides of the attention hand-over at 128): the step of forward_decode_batch.
    With some rows unflagged the step runs through the mixed entry's own logits stage — still the existing attention dispatch — at
    mixed depths and, for the two shallow sequences alone, on the one-launch decode attention."""
    plan_mod, _ = planmod
    lens = [3, 127, 128, 130]
    m = model_with_ctx(pkg, "mid-llama", 200, seed=67)
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=160, n_seqs=4)
    oracles = [orc.COracle(m) for _ in range(4)]
    b = Mixed(orc, plan, oracles, m, seed=13)
    for seq, n in enumerate(lens):
        b.prefill(seq, n)
    toks = b.tokens(4)
    order = [2, 0, 3, 1]
    args = ([toks[s] for s in order], order, [lens[s] for s in order])
    want_l, want_i = plan.forward_decode_batch(*args)
    got_l, got_i = plan.forward_batch(*args)
    assert np.array_equal(got_l, want_l) and np.array_equal(got_i, want_i)
    x_last = x_of_row(oracles[order[-1]], toks[order[-1]], lens[order[-1]])
    for row, s in enumerate(order):
        assert np.array_equal(want_l[row], oracles[s].forward(toks[s], lens[s])), s
    assert np.array_equal(plan.x(), x_last), "x of the last row"
    flags = [1, 0, 1, 1]
    got_l, got_i = plan.forward_batch(*args, want_logits=flags)
    keep = [r for r in range(4) if flags[r]]
    assert np.array_equal(got_l, want_l[keep]) and np.array_equal(got_i, want_i[keep])
    shallow = [1, 3]                                         # rows of sequences 0 and 1: positions 3 and 127
    got_l, got_i = plan.forward_batch(*[[a[r] for r in shallow] for a in args], want_logits=[0, 1])
    assert np.array_equal(got_l, want_l[[3]]) and np.array_equal(got_i, want_i[[3]])
    for s in range(4):
        for l in range(m.cfg.n_layers):
            k, v = plan.kv_seq(s, l, lens[s])
            ko, vo = oracles[s].kv(l, lens[s])
            assert np.array_equal(k, ko) and np.array_equal(v, vo), (s, l)
    plan.freeTornadoExecutionPlan()


def test_no_output_rows(pkg, orc, planmod):
    """Two runs with an all-zero want_logits and NULL outputs: a pure two-sequence prefill.  The decode step that follows reads the KV rows
    of both runs."""
    plan_mod, hip = planmod
    m = variant(pkg, "mid-llama", seed=69)
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=64, n_seqs=2)
    oracles = [orc.COracle(m) for _ in range(2)]
    rng = np.random.default_rng(15)
    prompts = [rng.integers(0, m.cfg.vocab, n).tolist() for n in (6, 11)]
    toks, seqs, poss = prompts[0] + prompts[1], [0] * 6 + [1] * 11, list(range(6)) + list(range(11))
    logits, ids = plan.forward_batch(toks, seqs, poss, want_logits=[0] * 17)
    assert logits is None and ids.size == 0
    t = np.ascontiguousarray(toks, np.int32); s = np.ascontiguousarray(seqs, np.int32); p = np.ascontiguousarray(poss, np.int32)
    w = np.zeros(17, np.int8)
    ptr = lambda a: a.ctypes.data_as(__import__("ctypes").c_void_p)
    assert hip.lib().gl3_forward_batch_sample(plan._ctx, ptr(t), ptr(s), ptr(p), ptr(w), 17, None, None, None, None) == 0      # nothing to sample
    for s_ in range(2):
        oracles[s_].prefill(prompts[s_], 0)
    nxt = rng.integers(0, m.cfg.vocab, 2).tolist()
    logits, ids = plan.forward_decode_batch(nxt, [0, 1], [6, 11])
    for s_ in range(2):
        ref = oracles[s_].forward(nxt[s_], len(prompts[s_]))
        assert np.array_equal(logits[s_], ref) and ids[s_] == orc.argmax(ref), s_
    plan.freeTornadoExecutionPlan()


def test_table_steps_around_graph_replayed_decode_steps(pkg, orc, planmod):
    """On one plan: runs of 5 and 3 rows (the run-table attention), a static-batched decode step of both sequences below position 128 (captured
    as a graph behind the first table step, replayed behind the second), and a third table step behind the replay.  A step's shape travels
    with the step: the decode steps take the one-launch attention and the graph although a table step ran before them, and the table steps
    take the table although a replayed graph ran before them.  The test guards results only (every row bit for bit against the oracle): the
    API does not say which attention kernel ran or whether a graph was replayed, and a step that kept another step's shape shows here as
    wrong logits, not as a wrong path."""
    plan_mod, _ = planmod
    m = variant(pkg, "tiny-llama", seed=73)
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=16, n_seqs=2)
    oracles = [orc.COracle(m) for _ in range(2)]
    b = Mixed(orc, plan, oracles, m, seed=23)
    for _ in range(2):
        b.step([(0, b.tokens(5)), (1, b.tokens(3))])
        toks = [b.next_id[0], b.next_id[1]]
        logits, ids = plan.forward_decode_batch(toks, [0, 1], list(b.pos))
        for s in range(2):
            ref = oracles[s].forward(toks[s], b.pos[s])
            assert np.array_equal(logits[s], ref) and ids[s] == orc.argmax(ref), (s, b.pos[s])
            b.pos[s] += 1
    b.step([(0, b.tokens(5)), (1, b.tokens(3))])
    assert b.pos == [17, 11]
    plan.freeTornadoExecutionPlan()


def test_sampled(pkg, orc, planmod):
    """One forward_batch_sample with four output rows — top-p, categorical, greedy, top-p (SETTINGS[0..3]) — the first and the last the ends
    of multi-row runs; ids and the probabilities they were drawn from equal the oracle's sampler on the oracle's logits."""
    plan_mod, hip = planmod
    assert [is_topp(*s) for s in SETTINGS[:4]] == [True, False, False, True] and SETTINGS[2][0] == 0 and SETTINGS[1][0] > 0
    m = variant(pkg, "mid-llama", seed=83)
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=64, n_seqs=4)
    oracles = [orc.COracle(m) for _ in range(4)]
    b = Mixed(orc, plan, oracles, m, seed=17)
    b.prefill(1, 3); b.prefill(2, 4)
    runs = [(0, b.tokens(5)), (1, b.tokens(1)), (2, b.tokens(1)), (3, b.tokens(7))]
    toks, seqs, poss, want = b.arrays(runs)
    jr = pkg.javarand.L32X64MixRandom(1234)
    coins = [jr.next_float() if SETTINGS[i][0] > 0 else 0.0 for i in range(4)]
    before = sum(plan.topp_counts())
    ids = plan.forward_batch_sample(toks, seqs, poss, [s[0] for s in SETTINGS[:4]], [s[1] for s in SETTINGS[:4]], coins)
    assert ids.dtype == np.int32 and ids.shape == (4,)
    out = 0
    for row in range(len(toks)):
        logits = oracles[seqs[row]].forward(toks[row], poss[row])
        if not want[row]:
            continue
        temperature, topp = SETTINGS[out]
        if temperature > 0:
            ref, probs = orc.sample(logits, temperature, topp, coins[out], want_probs=True)
            assert np.array_equal(plan.sample_probs_row(out), probs), out
        else:
            ref = orc.argmax(logits)
            with pytest.raises(hip.Gl3Error):
                plan.sample_probs_row(out)
        assert ids[out] == ref, (out, temperature, topp)
        out += 1
    assert out == 4 and sum(plan.topp_counts()) == before + 2
    plan.freeTornadoExecutionPlan()


def test_refusals_on_a_live_plan(pkg, orc, planmod):
    """A split run, a position gap and n > max_batch are argument errors; the correct step that follows matches the oracles: nothing of the
    refused steps was enqueued."""
    plan_mod, hip = planmod
    m = variant(pkg, "tiny-llama", seed=71)
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=16, n_seqs=3)
    b = Mixed(orc, plan, [orc.COracle(m) for _ in range(3)], m, seed=19)
    for toks, seqs, poss in (([1, 2, 3, 4], [0, 0, 1, 0], [0, 1, 0, 2]),                      # sequence 0 in two runs
                             ([1, 2, 3], [0, 0, 1], [0, 2, 0]),                               # a gap
                             (list(range(17)), [0] * 17, list(range(17)))):                   # n > max_batch
        with pytest.raises(hip.Gl3Error) as ei:
            plan.forward_batch(toks, seqs, poss)
        assert ei.value.code == hip.E_ARG == -1
        with pytest.raises(hip.Gl3Error) as ei:
            plan.forward_batch_sample(toks, seqs, poss, 0.7, 0.9, 0.5)
        assert ei.value.code == -1
    b.step([(0, b.tokens(9)), (1, b.tokens(2))])
    b.step([(2, b.tokens(3)), (0, [b.next_id[0]])])
    plan.freeTornadoExecutionPlan()


def test_native_host(pkg, orc, tmp_path):
    """gl3_batch_run -np 2 -b 16 -n 12 with prompts of 5, 21 and 9 ids: the second prompt spans two steps (16 rows less the first prompt's 5),
    the third waits for a slot and reuses it from position 0.  Every request's ids are the greedy ids of its prompt alone."""
    m = pkg.synth.make_numpy(pkg.synth.CONFIGS["tiny-llama"], seed=31)
    path = str(tmp_path / "m.gguf")
    m.write_gguf(path)
    rng = np.random.default_rng(21)
    prompts = [rng.integers(0, m.cfg.vocab, n).tolist() for n in (5, 21, 9)]
    pfile = tmp_path / "prompts.txt"
    pfile.write_text("".join(",".join(map(str, p)) + "\n" for p in prompts))

    def run(prompts_path, slots):
        return subprocess.run([EXE, "-m", path, "--prompts", str(prompts_path), "-np", str(slots), "-b", "16", "-n", "12"], capture_output=True, text=True, timeout=180)
    out = run(pfile, 2)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 3
    gm = pkg.synth.SynthModel.from_gguf(path)
    for k, prompt in enumerate(prompts):
        o = orc.COracle(gm)
        o.prefill(prompt[:-1], 0)
        want, cur, pos = [], prompt[-1], len(prompt) - 1
        while len(want) < 12:
            cur = orc.argmax(o.forward(cur, pos))
            want.append(cur)
            pos += 1
        head, _, rest = lines[k].partition(":")
        assert head == "request %d" % k and [int(x) for x in rest.split()] == want, k
    bad = tmp_path / "bad.txt"
    bad.write_text("1,2,3\n4,x,6\n")
    assert run(bad, 2).returncode == 2
    assert run(pfile, 0).returncode == 2
