"""gl3_kv_seq_copy (prefix fork): the K / V rows [p0, p1) of one sequence slot copied to the same positions of other slots.

A row's arithmetic does not depend on which rows share its step, so the K / V rows at positions 0 .. p of a sequence are a function of its
tokens 0 .. p alone and a copied prefix is bit for bit what forwarding it would have written.  Every comparison is np.array_equal on f32: the
copied rows against the source's, everything around them against a snapshot taken before the call, and the steps that follow a fork against
one CPU oracle per sequence that ran the prefix itself (Mixed.step of test_gpu_mixed_batch.py: logits, ids, x and the K / V rows the step
wrote)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
from test_gpu_batch_decode_depth import model_with_ctx
from test_gpu_mixed_batch import Mixed, oracle_for, variant

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tools", "gl3_batch_run")


@pytest.fixture(scope="module")
def planmod():
    from importlib import import_module
    ge.load_package()
    return import_module(ge.PKG_NAME + ".plan"), import_module(ge.PKG_NAME + ".hip")


def snapshot(plan, n_seqs, n_layers, rows):
    """[seq][layer][K | V][row][kv_dim] through the blocking tap"""
    return np.array([[[[plan.kv_seq(s, l, p)[kv] for p in range(rows)] for kv in (0, 1)] for l in range(n_layers)] for s in range(n_seqs)])


@pytest.mark.parametrize("cfg", ["mid-llama", "mid-qwen3"])
def test_copy_is_exact_and_touches_nothing_else(pkg, planmod, cfg):
    """Rows [3, 17) (odd start, 14 rows: 1.75 / 3.5 chunks of the kernel, so a guarded tail), [0, 1) (less than one chunk) and [0, 21) of
    sequence 0 into the unordered list [3, 1], over destinations that hold other, non-zero rows.  All 32 first rows of all four sequences are
    compared after every call: the copied ones with the source, every other one (rows 2 and 17 among them, sequences 0 and 2 whole) with the
    snapshot taken before the call."""
    plan_mod, _ = planmod
    m = model_with_ctx(pkg, cfg, 64, seed=81)
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=32, n_seqs=4)
    rng = np.random.default_rng(23)
    plan.prefill_seq(0, rng.integers(0, m.cfg.vocab, 21).tolist(), 0)
    for s in (1, 2, 3):
        plan.prefill_seq(s, rng.integers(0, m.cfg.vocab, 30).tolist(), 0)
    rows = 32
    before = snapshot(plan, 4, m.cfg.n_layers, rows)
    assert all(before[s, :, :, :21].any() for s in range(4)) and not np.array_equal(before[0, :, :, :21], before[1, :, :, :21]), "non-zero stale rows"
    for p0, p1 in ((3, 17), (0, 1), (0, 21)):
        plan.kv_seq_copy(0, [3, 1], p0, p1)
        after = snapshot(plan, 4, m.cfg.n_layers, rows)
        want = before.copy()
        for s in (1, 3):
            want[s, :, :, p0:p1] = before[0, :, :, p0:p1]
        for s in range(4):
            for l in range(m.cfg.n_layers):
                for kv in (0, 1):
                    for p in range(rows):
                        assert np.array_equal(after[s, l, kv, p], want[s, l, kv, p]), ("range", p0, p1, "seq", s, "layer", l, "KV"[kv], "row", p)
        before = after
    plan.freeTornadoExecutionPlan()


def fork(b, n_prefix, through_a_step):
    """A prompt of n_prefix tokens on sequence 0 (through a mixed step, or through prefill_seq); the oracles of the other sequences run the
    prompt themselves, the plan's other sequences get its rows by gl3_kv_seq_copy."""
    prompt = b.tokens(n_prefix)
    if through_a_step:
        b.step([(0, prompt)])
    else:
        b.plan.prefill_seq(0, prompt, 0)
        b.oracles[0].prefill(prompt, 0)
        b.pos[0] = n_prefix
    others = list(range(1, len(b.oracles)))
    for k in others:
        b.oracles[k].prefill(prompt, 0)
        b.pos[k] = n_prefix
    b.plan.kv_seq_copy(0, others, 0, n_prefix)
    for k in others:                                                   # the forked rows themselves: first, middle, last
        for p in sorted({0, n_prefix // 2, n_prefix - 1}):
            for l in range(b.m.cfg.n_layers):
                kp, vp = b.plan.kv_seq(k, l, p)
                ko, vo = b.oracles[k].kv(l, p)
                assert np.array_equal(kp, ko) and np.array_equal(vp, vo), ("forked kv", "seq", k, "layer", l, "pos", p)


def test_forked_sequences_continue_as_the_oracle_says(pkg, orc, planmod):
    """19 rows (not a multiple of the 8-row attention tile) forked to two sequences; then one step with a decode row on the source, a 5-token
    run on one fork and a different single token on the other, and one all-decode step."""
    plan_mod, _ = planmod
    m = variant(pkg, "mid-llama", seed=83)
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=64, n_seqs=3)
    b = Mixed(orc, plan, [oracle_for(orc, m, 8) for _ in range(3)], m, seed=27)
    fork(b, 19, through_a_step=True)
    other = b.tokens(1)
    while other[0] == b.next_id[0]:
        other = b.tokens(1)
    b.step([(0, [b.next_id[0]]), (1, b.tokens(5)), (2, other)])
    b.step([(s, [b.next_id[s]]) for s in range(3)])
    assert b.pos == [21, 25, 21]
    plan.freeTornadoExecutionPlan()


def test_fork_at_a_depth_of_the_long_context_attention(pkg, orc, planmod):
    """301 rows forked to one sequence, then a 9-row run on it: its rows sit past position 300, where a batched step's attention reads the
    forked rows through the tiled / long-context kernels (gl3_get_attn_rows tells which form served the step)."""
    plan_mod, _ = planmod
    m = model_with_ctx(pkg, "tiny-llama", 320, seed=85)
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=64, n_seqs=2)
    b = Mixed(orc, plan, [orc.COracle(m) for _ in range(2)], m, seed=29)
    fork(b, 301, through_a_step=False)
    b.step([(1, b.tokens(9))])
    rows = plan.attn_rows()
    assert sum(rows) == 9 and rows[1] + rows[2] > 0, rows
    assert b.pos == [301, 310]
    plan.freeTornadoExecutionPlan()


def test_more_chunks_than_the_grid_holds(pkg, planmod):
    """2304 rows of kv_dim 1024 over 2 layers are 2304 chunks of 16 KiB: more than the grid's cap of 8 workgroups per CU (2048 on 256 CUs), so
    workgroups take a second trip of the grid-stride loop.  Rows from both trips, the first and the last row, and the untouched row behind
    the range."""
    plan_mod, _ = planmod
    n = 2304
    m = model_with_ctx(pkg, "mid-qwen3", n + 16, seed=87)
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=256, n_seqs=2)
    rng = np.random.default_rng(31)
    plan.prefill_seq(0, rng.integers(0, m.cfg.vocab, n + 1).tolist(), 0)
    plan.kv_seq_copy(0, [1], 0, n)
    for l in range(m.cfg.n_layers):
        for p in (0, 1, 3, 4, 1023, 1151, 1152, 2047, 2048, 2049, 2300, n - 1):
            k, v = plan.kv_seq(1, l, p)
            ks, vs = plan.kv_seq(0, l, p)
            assert ks.any() and vs.any()
            assert np.array_equal(k, ks) and np.array_equal(v, vs), ("layer", l, "row", p)
        k, v = plan.kv_seq(1, l, n)
        assert not k.any() and not v.any(), ("row behind the range", l)
        assert plan.kv_seq(0, l, n)[0].any()
    plan.freeTornadoExecutionPlan()


def test_argument_checks(pkg, planmod):
    """Every refusal is GL3_E_ARG with a message, before anything is enqueued: a row of a would-be destination is unchanged afterwards.  An
    empty range is a valid no-op; a plan that is not finalized yet answers GL3_E_STATE."""
    plan_mod, hip = planmod
    m = variant(pkg, "tiny-llama", seed=89)
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=16, n_seqs=3)
    L, ctx = hip.lib(), m.cfg.ctx
    rng = np.random.default_rng(33)
    for s in range(3):
        plan.prefill_seq(s, rng.integers(0, m.cfg.vocab, 8).tolist(), 0)
    k_before = plan.kv_seq(1, 1, 4)[0].copy()
    assert k_before.any()

    def call(c, src, dsts, p0, p1, n_dst=None):
        d = np.ascontiguousarray(dsts, np.int32) if dsts is not None else None
        return L.gl3_kv_seq_copy(c, src, d.ctypes.data_as(C.c_void_p) if d is not None else None, len(dsts) if n_dst is None else n_dst, p0, p1)
    bad = [(None, 0, [1], 0, 8, None),            # null ctx
           (plan._ctx, 0, None, 0, 8, 1),         # null dst_seqs
           (plan._ctx, 0, [1], 0, 8, 0),          # n_dst <= 0
           (plan._ctx, 0, [1], 0, 8, -1),
           (plan._ctx, -1, [1], 0, 8, None),      # source outside [0, n_seqs)
           (plan._ctx, 3, [1], 0, 8, None),
           (plan._ctx, 0, [1, 3], 0, 8, None),    # a destination outside
           (plan._ctx, 0, [-1], 0, 8, None),
           (plan._ctx, 0, [1, 0], 0, 8, None),    # a destination equal to the source
           (plan._ctx, 0, [1, 2, 1], 0, 8, None),  # a destination listed twice
           (plan._ctx, 0, [1], -1, 8, None),      # p0 < 0
           (plan._ctx, 0, [1], 0, ctx + 1, None),  # p1 > ctx
           (plan._ctx, 0, [1], 5, 4, None)]       # p0 > p1
    for c, src, dsts, p0, p1, n_dst in bad:
        assert call(c, src, dsts, p0, p1, n_dst) == hip.E_ARG == -1, (src, dsts, p0, p1, n_dst)
        assert L.gl3_last_error(c), (src, dsts, p0, p1, n_dst)
    with pytest.raises(hip.Gl3Error) as ei:
        plan.kv_seq_copy(0, [1, 1], 0, 8)
    assert ei.value.code == -1
    assert np.array_equal(plan.kv_seq(1, 1, 4)[0], k_before)
    assert call(plan._ctx, 0, [1], 4, 4) == 0 and call(plan._ctx, 0, [1, 2], ctx, ctx) == 0
    assert np.array_equal(plan.kv_seq(1, 1, 4)[0], k_before)
    plan.kv_seq_copy(0, [1], 0, ctx)                                   # the whole context is a valid range
    assert np.array_equal(plan.kv_seq(1, 1, 4)[0], plan.kv_seq(0, 1, 4)[0]) and not np.array_equal(plan.kv_seq(1, 1, 4)[0], k_before)
    plan.freeTornadoExecutionPlan()

    c = m.cfg
    d = hip.ModelDesc(C.sizeof(hip.ModelDesc), c.arch, c.dim, c.hidden, c.n_layers, c.n_heads, c.n_kv_heads, c.head_size, c.vocab, c.ctx,
                      c.rms_eps, m.wtype, 1, 0, 0, 1, 0, 2, 1.0, 0.0, 1.0, 1.0, 0, 0, 0)
    raw = C.c_void_p()
    hip.check(L.gl3_create(C.byref(d), C.byref(raw)))
    try:
        assert call(raw, 0, [1], 0, 4) == hip.E_STATE == -6 and L.gl3_last_error(raw)
    finally:
        L.gl3_destroy(raw)


def test_native_host_shares_prefixes(pkg, orc, tmp_path):
    """gl3_batch_run -np 2 -b 64 -n 6 over P+a, Q, P+b, P+c (22 ids each, P = 19 ids): requests 0 and 1 finish in the same step; request 2
    re-enters slot 0, which still holds P's rows (19 in place); request 3 gets them copied from slot 0 into slot 1 (19 rows, one call).  The
    ids are the same with and without --share-prefix and equal every request's own oracle run; the flag saves exactly 38 rows."""
    m = pkg.synth.make_numpy(pkg.synth.CONFIGS["tiny-llama"], seed=35)
    path = str(tmp_path / "m.gguf")
    m.write_gguf(path)
    rng = np.random.default_rng(37)
    v = m.cfg.vocab
    P = rng.integers(0, v, 19).tolist()
    Q = rng.integers(0, v, 22).tolist()
    Q[0] = (P[0] + 1) % v                                              # unrelated: no common prefix at all
    firsts = [(P[0] + 2 + i) % v for i in range(3)]                    # distinct first ids of the tails
    a, b_, c = ([f] + rng.integers(0, v, 2).tolist() for f in firsts)
    prompts = [P + a, Q, P + b_, P + c]
    assert all(len(p) == 22 for p in prompts)
    pfile = tmp_path / "prompts.txt"
    pfile.write_text("".join(",".join(map(str, p)) + "\n" for p in prompts))

    def run(*extra):
        out = subprocess.run([EXE, "-m", path, "--prompts", str(pfile), "-np", "2", "-b", "64", "-n", "6", *extra], capture_output=True, text=True, timeout=180)
        assert out.returncode == 0, out.stderr
        return out
    plain, shared = run(), run("--share-prefix")
    assert plain.stdout == shared.stdout
    lines = plain.stdout.strip().splitlines()
    assert len(lines) == 4
    gm = pkg.synth.SynthModel.from_gguf(path)
    for k, prompt in enumerate(prompts):
        o = orc.COracle(gm)
        o.prefill(prompt[:-1], 0)
        want, cur, pos = [], prompt[-1], len(prompt) - 1
        while len(want) < 6:
            cur = orc.argmax(o.forward(cur, pos))
            want.append(cur)
            pos += 1
        head, _, rest = lines[k].partition(":")
        assert head == "request %d" % k and [int(x) for x in rest.split()] == want, k
    assert "prefix rows reused" not in plain.stderr
    assert "prefix rows reused: 38 (19 copied in 1 calls, 19 in place)" in shared.stderr, shared.stderr

    def rows(err):
        return int(re.search(r", (\d+) rows in ", err).group(1))
    assert rows(plain.stderr) == 4 * 22 + 4 * 5 and rows(shared.stderr) == rows(plain.stderr) - 38, (plain.stderr, shared.stderr)
