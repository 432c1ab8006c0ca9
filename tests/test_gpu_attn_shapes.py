"""Attention at every head size and kvMul that gl3_create accepts: the shape grid of tests/attn_shapes.py through single-token decode in all its
regimes, static-batched decode and mixed steps, bit for bit (np.array_equal on f32) against one CPU oracle per sequence.

Which kernels a case runs follows from (head size, kvMul, depth); attn_shapes.py restates the rule and the tests assert it by plan.attn_rows()
where that tap tells the forms apart (batched and mixed steps, prefill chunks).  Single-token decode has no tap: there the rule is

    position < 128 and attn_head_smem(head size) <= 150 KB (head size <= 128), no GL3_NO_FUSED_ATTN    attn_head_kernel, one query head per workgroup
    else position < 768 (attn_mid)                         attn_scores_kernel (64 x kvMul threads, LDS (kvMul hs + 64 (hs + 4) + hs) floats)
                                                           + attn_softmax_pv_kernel
    else                                                   kvMul <= 4 and head size 64 | 128: attn_scores_loop_kernel<hs> (kvMul chain wavefronts),
                                                           otherwise attn_scores_kernel; then attn_exp_kernel, attn_sum_kernel (att_t in
                                                           [kv head][head quad][t][4] order) and attn_pv_kernel (ceil(kvMul / 4) head quads)

(csrc/gl3_decode_attn.h: attn_regime, attn_plan; tests/test_attn_shapes.py holds decode_regime equal to it), so a decode step at position p of shape s runs the kernels decode_regime(hs, kvMul, p) names — the
positions of the walk meet every regime a shape has (tests/test_attn_shapes.py)."""
import os

import numpy as np
import pytest

import attn_shapes as sh
from test_gpu_batch_decode_depth import Batch, rotated
from test_gpu_mixed_batch import Mixed, planmod, schedule  # noqa: F401  (planmod: a fixture)

pytestmark = pytest.mark.gpu

CTX, DECODE_AT, PREFILL_KV_AT = sh.CTX, sh.DECODE_AT, sh.PREFILL_KV_AT
CHUNK = 256
ALL = sorted(sh.SHAPES)
WIDE = [n for n in ALL if sh.kvmul_of(n) >= 5 and sh.has_head_kernel(sh.head_size_of(n))]      # kvMul 5 - 16 at head sizes with attn_head_kernel
LARGE = [n for n in ALL if not sh.has_head_kernel(sh.head_size_of(n))]                        # head sizes 160 - 256


class Reference:
    """One shape's model, token stream and oracle results along the walk: logits of every decode position, K / V rows of the decode positions
    and of PREFILL_KV_AT in every layer.  Computed once per shape and read by every test of the shape."""

    def __init__(self, pkg, orc, name):
        self.name, self.hs, self.kvmul = name, sh.head_size_of(name), sh.kvmul_of(name)
        self.m = m = sh.shape_model(pkg, name, CTX, seed=41)
        assert (m.cfg.head_size, m.cfg.n_heads // m.cfg.n_kv_heads) == (self.hs, self.kvmul)
        self.toks = pkg.javarand.bench_tokens(m.cfg.vocab, CTX)
        o = orc.COracle(m)
        self.logits, done = {}, 0
        for p in DECODE_AT:
            if done < p:
                o.prefill(self.toks[done:p], done)
            self.logits[p] = o.forward(self.toks[p], p)
            done = p + 1
        self.kv = {(l, p): o.kv(l, p) for l in range(m.cfg.n_layers) for p in DECODE_AT + PREFILL_KV_AT}
        for a in list(self.logits.values()) + [r for kv in self.kv.values() for r in kv]:
            a.setflags(write=False)
        o.close()


_REFS = {}


def reference(pkg, orc, name):
    if name not in _REFS:
        _REFS[name] = Reference(pkg, orc, name)
    return _REFS[name]


def walk(plan, ref, decode_at, pair_prefill):
    """Batched prefill up to each decode position in chunks of CHUNK (122, 256 + 256 + 123 and 256 + 4 rows at non-zero positions), decode steps at
    `decode_at`; logits of every step, then K / V rows of every layer.  pair_prefill: the shape's prompt rows run on the per-row pair."""
    done = 0
    for p in decode_at:
        while done < p:
            n = min(CHUNK, p - done)
            plan.tornadoVMForwardBatchPrefill(ref.toks[done:done + n], done)
            rows = plan.attn_rows()
            assert sum(rows) == n and rows[0] == 0 and rows[3] == (n if pair_prefill else 0), (ref.name, done, n, rows)
            done += n
        got = plan.forward_decode(ref.toks[p], p)
        assert np.array_equal(got, ref.logits[p]), (ref.name, "logits", p, sh.decode_regime(ref.hs, ref.kvmul, p))
        done = p + 1
    checked = 0
    for (l, p), (ko, vo) in sorted(ref.kv.items()):
        if p < done:
            k, v = plan.kv(l, p)
            assert np.array_equal(k, ko) and np.array_equal(v, vo), (ref.name, "kv", "layer", l, "pos", p, "decode" if p in decode_at else "prefill")
            checked += 1
    assert checked >= 2 * len(decode_at)


def plan_under(plan_mod, m, env, **kw):
    """A plan made with `env` set: GL3_NO_FUSED_ATTN and GL3_ATTN_WINDOW are read in gl3_create"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return plan_mod.HipMasterPlan(m, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ---- 1. single-token decode through all regimes
@pytest.mark.parametrize("name", ALL)
def test_decode_through_all_regimes(pkg, orc, planmod, name):
    """Positions 0 - 3 and 126 - 127: attn_head_kernel (head size <= 128) or the pair from position 0 (head size >= 160: qk-norm, RoPE and the
    strided K / V write over up to 256 elements on 64-lane wavefronts).  128 - 130 and 766 - 767: the pair, 3 and 12 score tiles.  768 - 769 and
    1030 - 1031: the four-launch path — at kvMul 2 / 3 and head size 64 / 128 the looping scores kernel, at every other shape attn_scores_kernel
    with 64 x kvMul threads (1024 at kvMul 16; 82 KB of LDS at head size 256) — with att_t written in head quads (ragged at kvMul 5 and 7:
    surplus heads clamped in attn_pv_kernel) past PV_ROWS.  The prompt rows between them are the shape's prefill coverage: tiled kernels at head
    sizes 32 / 64 / 128 (no row on the per-row pair), pf_rope_kv_kernel + pf_attn_scores_kernel + pf_attn_softmax_pv_kernel on every row at
    head sizes 160 - 256."""
    plan_mod, _ = planmod
    ref = reference(pkg, orc, name)
    plan = plan_mod.HipMasterPlan(ref.m, prefill_batch_size=CHUNK)
    walk(plan, ref, DECODE_AT, pair_prefill=not sh.has_tiled_prefill(ref.hs, ref.kvmul))
    plan.freeTornadoExecutionPlan()


@pytest.mark.parametrize("name", ["llama-hs256-kv16", "llama-hs128-kv16"])
def test_decode_with_windowed_softmax_rows(pkg, orc, planmod, name):
    """GL3_ATTN_WINDOW=1024 on a context of 1100: the softmax row of attn_softmax_pv_kernel is 1024 floats, and so is that of the per-row prefill
    kernel, whose rows from position 1024 on (head size 256) run in two windows with the sequential sum carried across.  Same walk, same
    reference."""
    plan_mod, _ = planmod
    ref = reference(pkg, orc, name)
    assert (ref.hs == 256 or ref.kvmul == 16) and CTX > 1024
    plan = plan_under(plan_mod, ref.m, {"GL3_ATTN_WINDOW": "1024"}, prefill_batch_size=CHUNK)
    walk(plan, ref, DECODE_AT, pair_prefill=not sh.has_tiled_prefill(ref.hs, ref.kvmul))
    plan.freeTornadoExecutionPlan()


@pytest.mark.parametrize("name", WIDE)
def test_wide_groups_on_the_pair_from_position_0(pkg, orc, planmod, name):
    """GL3_NO_FUSED_ATTN=1: kvMul 5 - 16 at head sizes 32 / 64 / 128 run attn_scores_kernel + attn_softmax_pv_kernel at positions 0 - 3 and
    126 - 130 too (one and two score tiles, the owner workgroup's K / V write at 64 x kvMul threads)."""
    plan_mod, _ = planmod
    ref = reference(pkg, orc, name)
    shallow = [p for p in DECODE_AT if p <= 130]
    assert {sh.decode_regime(ref.hs, ref.kvmul, p, head_kernel=False) for p in shallow} == {"pair"} and len(shallow) == 9
    plan = plan_under(plan_mod, ref.m, {"GL3_NO_FUSED_ATTN": "1"}, prefill_batch_size=CHUNK)
    walk(plan, ref, shallow, pair_prefill=False)
    plan.freeTornadoExecutionPlan()


# ---- 2. static-batched decode
LENS = [3, 60, 125, 126, 127]
BATCH_CASES = [(n, 8) for n in WIDE + LARGE] + [("llama-hs64-kv8", 1)]


def batched_steps(b, hs):
    """Two steps with every row below 128 (all five rows: 3 .. 127; then the three shallowest), then three that carry rows across 128 in changing
    row order.  attn_rows() of every step against the rule."""
    plan, taps = b.plan, []
    for step, members in enumerate(([0, 1, 2, 3, 4], [0, 1, 2], [0, 1, 2, 3, 4], [4, 3, 2, 1, 0], [2, 3, 4])):
        order = rotated(members, step)
        want = sh.batched_rows(hs, [b.pos[s] for s in order])
        b.step(order)
        taps.append(plan.attn_rows())
        assert taps[-1] == want, (step, taps[-1], want, b.log[-1])
    deep = [max(at) >= sh.AF_MAXN for _, at in b.log]
    assert deep == [False, False, True, True, True] and b.log[0][1].count(127) == 1 and 128 in b.log[2][1] and min(b.log[3][1]) < 64
    assert any(127 in at and 128 in at for _, at in b.log), "no step with rows on both sides of 128"
    b.check_kv()
    return taps


@pytest.mark.parametrize("name,wtype", BATCH_CASES, ids=["%s-%d" % c for c in BATCH_CASES])
def test_static_batched_decode(pkg, orc, planmod, name, wtype):
    """Five sequences at depths 3, 60, 125, 126, 127.  Head sizes <= 128: the shallow steps run attn_head_kernel — one workgroup per (kv head,
    token) serving G = kvMul = 5, 7, 8 query heads (e[G][128] in LDS, softmax one wavefront per head), or at kvMul 16 one query head per
    workgroup, where h0 % kvMul == 0 picks the head that writes the K / V row — and the steps with a row at 128 or beyond the per-row kernels.
    Head sizes 160 - 256: the per-row kernels at every depth.  wtype 1: F16 weights in the 256-bit vector order; the attention output
    leaves attn_head_kernel as f32."""
    plan_mod, _ = planmod
    hs, kvmul = sh.head_size_of(name), sh.kvmul_of(name)
    m = sh.shape_model(pkg, name, 200, seed=43, wtype=wtype)
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=160, n_seqs=len(LENS))
    oracles = [orc.COracle(m, vector_bits=256) if wtype != 8 else orc.COracle(m) for _ in LENS]
    taps = batched_steps(Batch(orc, plan, oracles, m, LENS, seed=17, calls={2: [70, 55]}), hs)
    if sh.has_head_kernel(hs):
        assert taps[:2] == [[5, 0, 0, 0], [3, 0, 0, 0]] and sh.bd_group(hs, kvmul) == (kvmul if kvmul <= 8 else 1)
    else:
        assert taps[:2] == [[0, 0, 0, 5], [0, 0, 0, 3]]
    assert taps[2:] == [[0, 0, 0, 5], [0, 0, 0, 5], [0, 0, 0, 3]]
    plan.freeTornadoExecutionPlan()


# ---- 3. mixed steps
class Taps(Mixed):
    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.taps = []

    def step(self, runs, **k):
        super().step(runs, **k)
        self.taps.append(self.plan.attn_rows())


@pytest.mark.parametrize("name", LARGE)
def test_mixed_steps_on_the_per_row_pair(pkg, orc, planmod, name):
    """schedule() of test_gpu_mixed_batch.py (steps of 12, 19 and 8 rows, each with a run of several rows) at head sizes 160 - 256: no tiled
    kernel exists, every row of every step is on the per-row pair.  A tiled form for these head sizes has to change this on purpose."""
    plan_mod, _ = planmod
    m = sh.shape_model(pkg, name, 64, seed=61)
    assert not sh.has_tiled_prefill(m.cfg.head_size, sh.kvmul_of(name))
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=64, n_seqs=4)
    b = Taps(orc, plan, [orc.COracle(m) for _ in range(4)], m, seed=7)
    schedule(b)
    assert b.taps == [[0, 0, 0, 12], [0, 0, 0, 19], [0, 0, 0, 8]], b.taps
    plan.freeTornadoExecutionPlan()
