"""The mixed batched step at depth: a step's attention tiles are split by depth — the 8-row tiles whose score rows fit LDS run on the one-launch
tiled kernels (run-table form), the deeper rows on the run-table form of the long-context trio (scores -> pf_softmax_rows_kernel -> weighted V
sum over score rows in HBM) — so one deep decode row no longer sends a whole step to the per-row pair.

Every case compares logits, ids, x and K / V rows with np.array_equal against one CPU oracle per sequence (Mixed.step of
test_gpu_mixed_batch.py) and checks plan.attn_rows(): the rows of the step by the attention form that served them,
[attn_head_kernel, one-launch tiled kernels, long-context trio, per-row pair].

The limit between the two forms is derived from the kernels' LDS sizes (511 at head size 128 / kvMul 4).  GL3_PF_TAB_MAXPOS=<p> lowers it
(read once per process), so that contexts of 160 positions exercise the split: the schedule cases below run in this process with the limit
the shape has and once more in a child pytest under GL3_PF_TAB_MAXPOS=40; what attn_rows() must report is computed here from the schedule and
the limit in force."""
import os
import subprocess
import sys

import numpy as np
import pytest

import edge_models as em
from test_gpu_batch_decode_depth import model_with_ctx
from test_gpu_mixed_batch import Mixed, oracle_for, planmod, schedule, variant  # noqa: F401  (planmod: a fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_LIMIT = 1 << 30


def limit_of(cfg):
    """fused_max_pos of a shape at the contexts used here (<= 600 positions): -1 where the one-launch kernels do not exist (a K tile is more than
    8 float4 per thread: head size 128 below kvMul 4, head size 64 at kvMul 1), 511 at head size 128 / kvMul 4 (the documented limit), past
    any context used here otherwise; GL3_PF_TAB_MAXPOS lowers it."""
    kvmul = cfg.n_heads // cfg.n_kv_heads
    assert kvmul <= 4 and cfg.head_size in (32, 64, 128)
    own = -1 if 64 * (cfg.head_size // 4) > 8 * 64 * kvmul else 511 if (cfg.head_size, kvmul) == (128, 4) else NO_LIMIT
    env = os.environ.get("GL3_PF_TAB_MAXPOS")
    return min(own, int(env)) if env else own


def expected_rows(runs, limit):
    """runs [(first position, rows)] of a step with a run of several rows -> attn_rows(): a run's shallow rows are its leading 8-row tiles whose
    last position is <= limit"""
    n = deep = 0
    for pos0, rows in runs:
        o = 0
        while o < rows and pos0 + min(o + 8, rows) - 1 <= limit:
            o = min(o + 8, rows)
        n += rows
        deep += rows - o
    return [0, n - deep, deep, 0]


class Tapped(Mixed):
    """Mixed whose step() also checks attn_rows() against the split of the step's runs at `limit` (taps: what it reported)"""

    def __init__(self, *a, limit, **k):
        super().__init__(*a, **k)
        self.limit, self.taps = limit, []

    def step(self, runs, **k):
        want = expected_rows([(self.pos[seq], len(t)) for seq, t in runs], self.limit)
        super().step(runs, **k)
        got = self.plan.attn_rows()
        self.taps.append(got)
        assert got == want, (got, want, [(self.pos[seq] - len(t), len(t)) for seq, t in runs], self.limit)


# ---- at real depth, no switch
def test_decode_row_at_560_beside_a_prompt_run(pkg, orc, planmod):
    """mid-qwen3 (head size 128, kvMul 4): a decode row at position 560 and a 12-row prompt run.  The run's tiles keep the one-launch table
    form, the decode row alone takes the trio ([0, 12, 1, 0]; before the split all 13 rows ran on the per-row pair).  Around it the
    one-sequence prefill reports its chunks by depth, unchanged: one launch while the score rows of a tile fit LDS without the table form's
    query rows (a chunk ending at position 624 does, one ending at 660 does not); the decode row that follows reads those K / V rows."""
    plan_mod, _ = planmod
    m = model_with_ctx(pkg, "mid-qwen3", 704, seed=65)
    assert limit_of(m.cfg) == 511
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=64, n_seqs=2)
    b = Tapped(orc, plan, [orc.COracle(m) for _ in range(2)], m, seed=11, limit=limit_of(m.cfg))
    b.prefill(0, 64)
    assert plan.attn_rows() == [0, 64, 0, 0]
    b.prefill(0, 496)                            # chunks of 64 from position 64: the last one is rows 512..559
    assert plan.attn_rows() == [0, 48, 0, 0]
    b.step([(0, b.tokens(1)), (1, b.tokens(12))])
    assert b.pos == [561, 12] and b.taps == [[0, 12, 1, 0]]
    b.prefill(0, 64)                             # rows 561..624
    assert plan.attn_rows() == [0, 64, 0, 0]
    b.prefill(0, 36)                             # rows 625..660
    assert plan.attn_rows() == [0, 0, 36, 0]
    b.step([(1, b.tokens(3)), (0, b.tokens(1))])
    assert b.pos == [662, 15] and b.taps[1] == [0, 3, 1, 0]
    plan.freeTornadoExecutionPlan()


def test_the_derived_limit_is_position_511(pkg, orc, planmod):
    """The same model: a step whose deepest row is at position 511 is all on the one-launch table form, one whose deepest row is at 512 has
    that row on the trio and nothing on the pair."""
    plan_mod, _ = planmod
    m = model_with_ctx(pkg, "mid-qwen3", 600, seed=66)
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=64, n_seqs=2)
    b = Tapped(orc, plan, [orc.COracle(m) for _ in range(2)], m, seed=12, limit=511)
    b.prefill(0, 511)
    b.step([(0, b.tokens(1)), (1, b.tokens(12))])            # positions 511 and 0..11
    b.step([(1, b.tokens(5)), (0, [b.next_id[0]])])          # 12..16 and 512
    assert b.pos == [513, 17]
    assert b.taps[0] == [0, 13, 0, 0]
    assert b.taps[1][2] >= 1 and b.taps[1][3] == 0 and b.taps[1] == [0, 5, 1, 0]
    plan.freeTornadoExecutionPlan()


# ---- the split on short contexts: here with the shape's own limit, in a child pytest under GL3_PF_TAB_MAXPOS=40
def straddling_schedule(b):
    """94 rows (> 64: the chunk-major GEMMs consume the attention output, f32 in a split step): a 70-row run from position 20 that straddles
    the limit of 40 (tiles 20..27 and 28..35 shallow, 36..43 and on deep: 16 + 16 + 16 + 6 rows), a 21-row continuation chunk from position
    119 (deep; ragged against 16; crosses the K-tile boundary at 128), decode rows at depths 2, 45 and 130."""
    for seq, depth in ((0, 20), (1, 119), (2, 2), (3, 45), (4, 130)):
        b.prefill(seq, depth)
    b.step([(2, b.tokens(1)), (0, b.tokens(70)), (3, b.tokens(1)), (1, b.tokens(21)), (4, b.tokens(1))])
    assert b.pos == [90, 140, 3, 46, 131]
    if b.limit == 40:
        assert b.taps == [[0, 17, 77, 0]]


STRADDLE_CASES = [("mid-qwen3", 8, {}),                     # head size 128, kvMul 4: scores / V sum on the matrix pipe
                  ("mid-llama", 8, {}),                     # head size 64, kvMul 4: the matrix pipe
                  ("mid-llama", 8, {"n_kv_heads": 16}),     # kvMul 2: pf_scores_pk_kernel + pf_pv_ring_kernel
                  ("mid-phi3", 8, {}),                      # kvMul 3: pf_scores_tiled_kernel + ring; no one-launch kernel, every row deep at any limit
                  ("mid-llama", 1, {})]                     # F16: pf_layers_vl


@pytest.mark.parametrize("cfg,wtype,over", STRADDLE_CASES, ids=["%s-%d%s" % (c, w, "-kv%d" % o["n_kv_heads"] if "n_kv_heads" in o else "") for c, w, o in STRADDLE_CASES])
def test_straddling_schedule(pkg, orc, planmod, cfg, wtype, over):
    plan_mod, _ = planmod
    m = variant(pkg, cfg, seed=75, wtype=wtype, ctx=160, **over)
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=128, n_seqs=5)
    b = Tapped(orc, plan, [oracle_for(orc, m, wtype) for _ in range(5)], m, seed=29, limit=limit_of(m.cfg))
    straddling_schedule(b)
    if cfg == "mid-phi3":
        assert b.taps == [[0, 0, 94, 0]]
    plan.freeTornadoExecutionPlan()


def test_straddling_value_edges(pkg, orc, planmod):
    """The "all" edits of edge_models.py (peaked attention: softmax terms that are exactly 0 or f32-subnormal; ZERO_TOKEN as a query ties every
    score at the maximum) on tiny-qwen3 (head size 64, kvMul 4): a 60-row run from position 0 that straddles the limit with ZERO_TOKEN queries
    on both sides of it, deep decode rows at 45 (FLAT_TOKEN) and 50 (ZERO_TOKEN), a shallow 30-row run."""
    plan_mod, _ = planmod
    m = em.make_edge_model("tiny-qwen3", 8, 7, "all", ctx=160)
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=128, n_seqs=4)
    b = Tapped(orc, plan, [orc.COracle(m) for _ in range(4)], m, seed=19, limit=limit_of(m.cfg))
    b.prefill(0, 45)
    b.prefill(1, 50)
    c0, c1 = b.tokens(60), b.tokens(30)
    c0[0] = c0[7] = c0[8] = c0[50] = c0[59] = c1[0] = em.ZERO_TOKEN
    c0[1] = c0[44] = c1[3] = em.FLAT_TOKEN
    b.step([(0, [em.FLAT_TOKEN]), (2, c0), (1, [em.ZERO_TOKEN]), (3, c1)])
    assert b.pos == [46, 51, 60, 30]
    if b.limit == 40:
        assert b.taps == [[0, 70, 22, 0]]        # 40 + 30 shallow rows; 20 rows of the long run and the two decode rows deep
    plan.freeTornadoExecutionPlan()


def test_the_split_under_a_lowered_limit():
    """GL3_PF_TAB_MAXPOS=40 (read once per process): the six schedule cases above in a child pytest, where 77 of the 94 rows (22 of 92) are deep."""
    e = dict(os.environ, GL3_PF_TAB_MAXPOS="40")
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-k", "test_straddling", "-p", "no:cacheprovider"],
                         capture_output=True, text=True, timeout=600, env=e, cwd=ROOT)
    tail = out.stdout[-1500:] + out.stderr[-500:]
    assert out.returncode == 0, tail
    assert "6 passed" in out.stdout and "failed" not in out.stdout and "skipped" not in out.stdout, tail


# ---- a shape with tiled long-context kernels but no one-launch kernel
def test_qwen2moe_schedule_leaves_the_per_row_pair(pkg, orc, planmod):
    """mid-qwen2moe (16 / 16 heads of 128: kvMul 1): every step of the three-step schedule has a run of several rows and runs on the trio at
    any depth (before: the per-row pair)."""
    plan_mod, _ = planmod
    m = variant(pkg, "mid-qwen2moe", seed=61)
    assert limit_of(m.cfg) == -1
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=64, n_seqs=4)
    b = Tapped(orc, plan, [orc.COracle(m) for _ in range(4)], m, seed=7, limit=-1)
    schedule(b)
    assert b.taps == [[0, 0, 12, 0], [0, 0, 19, 0], [0, 0, 8, 0]] and all(t[3] == 0 for t in b.taps)
    plan.freeTornadoExecutionPlan()


# ---- unchanged paths
def test_single_row_steps_keep_their_dispatch(pkg, orc, planmod):
    """Steps of single rows: attn_head_kernel while every row is below position 128, the per-row pair with a row past it — through the mixed
    entry with every row flagged (the static-batched decode step) and with one row unflagged (the mixed entry's own logits stage)."""
    plan_mod, _ = planmod
    m = model_with_ctx(pkg, "mid-llama", 200, seed=67)
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=16, n_seqs=4)
    b = Mixed(orc, plan, [orc.COracle(m) for _ in range(4)], m, seed=13)
    for seq, n in enumerate((3, 126, 128, 130)):
        b.prefill(seq, n)
    b.step([(1, b.tokens(1)), (0, b.tokens(1))])                                    # positions 126 and 3
    assert plan.attn_rows() == [2, 0, 0, 0]
    b.step([(2, b.tokens(1)), (0, b.tokens(1)), (3, b.tokens(1)), (1, b.tokens(1))])        # 128, 4, 130, 127
    assert plan.attn_rows() == [0, 0, 0, 4]
    toks, seqs, poss, _ = b.arrays([(0, b.tokens(1)), (2, b.tokens(1))])              # 5 and 129, the first row unflagged
    logits, ids = plan.forward_batch(toks, seqs, poss, [0, 1])
    assert plan.attn_rows() == [0, 0, 0, 2]
    b.oracles[0].forward(toks[0], poss[0])
    assert np.array_equal(logits[0], b.oracles[2].forward(toks[1], poss[1]))
    b.pos[0] += 1; b.pos[2] += 1
    b.step([(0, b.tokens(1))])                                                      # position 6 alone: shallow again
    assert plan.attn_rows() == [1, 0, 0, 0]
    plan.freeTornadoExecutionPlan()


def test_attn_rows_before_any_batched_step(pkg, planmod):
    plan_mod, hip = planmod
    m = variant(pkg, "tiny-llama", seed=3)
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=16, n_seqs=2)
    with pytest.raises(hip.Gl3Error) as ei:
        plan.attn_rows()
    assert ei.value.code == -6                   # GL3_E_STATE
    plan.prefill_seq(0, [1, 2, 3], 0)
    assert plan.attn_rows() == [0, 3, 0, 0]
    plan.freeTornadoExecutionPlan()
