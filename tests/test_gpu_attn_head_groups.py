"""Tiled prefill attention in head groups (kvMul 5 - 16) and at head size 96.

A workgroup of the tiled kernels serves a head group: 4 consecutive query heads of one kv head, ceil(kvMul / 4) groups per kv head, the last one
ragged (1 - 4 real heads; its surplus head slots repeat the group's last real head and store nothing).  Head size 96 (Phi-3-mini) has the VALU
long-context kernels only, so every row of a step with a run takes the trio.  Nothing changes a result: every case compares logits, greedy ids,
x and K / V rows with np.array_equal against one CPU oracle per sequence (Mixed.step of test_gpu_mixed_batch.py) and checks plan.attn_rows():
[attn_head_kernel, one-launch tiled kernels, long-context trio, per-row pair].  Before head groups every case here reported [0, 0, 0, n].

The shapes (the CPU oracle accepts every override as written):
    a  mid-qwen2                                kvMul 6, head size 128: groups of 4 + 2, q/k/v bias
    b  mid-qwen3 + n_heads 28, n_kv_heads 4     kvMul 7, head size 128: 4 + 3
    c  mid-qwen3 + n_heads 20, n_kv_heads 4     kvMul 5, head size 128: 4 + 1
    d  mid-llama + n_kv_heads 4                 kvMul 8, head size 64: 4 + 4
    e  mid-llama + n_kv_heads 2                 kvMul 16, head size 64: four groups
    f  tiny-qwen3 + n_heads 14, n_kv_heads 2    kvMul 7, head size 64: 4 + 3
    g  tiny-llama + n_kv_heads 1                kvMul 8, head size 32: the VALU kernels (pf_attn_fused2_kernel<32>), one kv head
    h  phi3-hs96                                kvMul 1, head size 96: trio only
    i  phi3-hs96 + n_kv_heads 2                 kvMul 4, head size 96: trio only
    j  phi3-hs96 + n_kv_heads 1                 kvMul 8, head size 96: the group is orthogonal to the head size, so this is served too (trio)
Every shape but g has >= 2 kv heads, so kvh > 0 is indexed.  mid-qwen3's own context of 40 is below the 64 positions pf_softmax_rows_kernel
asks for; b and c run at 64 and above."""
import os
import subprocess
import sys

import numpy as np
import pytest

import edge_models as em
from test_gpu_batch_decode_depth import model_with_ctx  # noqa: F401  (the helper the depth tests share)
from test_gpu_mixed_batch import Mixed, oracle_for, planmod, schedule, variant  # noqa: F401  (planmod: a fixture)
from test_gpu_mixed_batch_depth import NO_LIMIT, Tapped, expected_rows, straddling_schedule

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = {"a": ("mid-qwen2", {}),
         "b": ("mid-qwen3", {"n_heads": 28, "n_kv_heads": 4}),
         "c": ("mid-qwen3", {"n_heads": 20, "n_kv_heads": 4}),
         "d": ("mid-llama", {"n_kv_heads": 4}),
         "e": ("mid-llama", {"n_kv_heads": 2}),
         "f": ("tiny-qwen3", {"n_heads": 14, "n_kv_heads": 2}),
         "g": ("tiny-llama", {"n_kv_heads": 1}),
         "h": ("phi3-hs96", {}),
         "i": ("phi3-hs96", {"n_kv_heads": 2}),
         "j": ("phi3-hs96", {"n_kv_heads": 1})}
KVMUL_HS = {"a": (6, 128), "b": (7, 128), "c": (5, 128), "d": (8, 64), "e": (16, 64), "f": (7, 64), "g": (8, 32), "h": (1, 96), "i": (4, 96),
            "j": (8, 96)}


def case_model(pkg, case, seed, ctx=None):
    cfg, over = CASES[case]
    base = pkg.synth.CONFIGS[cfg]
    m = variant(pkg, cfg, seed=seed, **over, ctx=ctx or max(base.ctx, 64))
    assert (m.cfg.n_heads // m.cfg.n_kv_heads, m.cfg.head_size) == KVMUL_HS[case] and m.cfg.n_layers == 2
    assert m.cfg.ctx % 4 == 0 and m.cfg.ctx >= 64          # pf_softmax_rows_kernel: without it these shapes keep the per-row pair
    return m


def limit_of(case):
    """fused_max_pos of a case: a head group is the kvMul-4 workgroup, so the limits are those of kvMul 4 at the head size — 511 at 128, past
    any context used here at 64 and 32 — and -1 at head size 96, which has no one-launch kernel.  GL3_PF_TAB_MAXPOS lowers it."""
    hs = KVMUL_HS[case][1]
    own = -1 if hs == 96 else 511 if hs == 128 else NO_LIMIT
    env = os.environ.get("GL3_PF_TAB_MAXPOS")
    return min(own, int(env)) if env else own


def child(env, select, passed):
    """A fresh pytest of this file under switches that are read once per process"""
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-k", select, "-p", "no:cacheprovider"],
                         capture_output=True, text=True, timeout=600, env=dict(os.environ, **env), cwd=ROOT)
    tail = out.stdout[-1500:] + out.stderr[-500:]
    assert out.returncode == 0, tail
    assert "%d passed" % passed in out.stdout and "failed" not in out.stdout and "skipped" not in out.stdout, tail


# ---- 1. the three-step schedule on every case
@pytest.mark.parametrize("case", sorted(CASES), ids=["case_%s" % c for c in sorted(CASES)])
def test_schedule_parity(pkg, orc, planmod, case):
    """Steps of 12, 19 and 8 rows, each with a run of several rows.  Head sizes 128 / 64 / 32 (a - g): every row on the one-launch table form —
    at head size 32 too: a group of 4 heads stages a K tile of 8 float4 rows with 8 slots per thread to spare, so pf_attn_fused2_kernel<32>
    serves case g as it serves kvMul 4.  Head size 96 (h, i, j): every row on the trio.  No row on the per-row pair."""
    plan_mod, _ = planmod
    m = case_model(pkg, case, seed=61)
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=64, n_seqs=4)
    b = Tapped(orc, plan, [orc.COracle(m) for _ in range(4)], m, seed=7, limit=limit_of(case))
    schedule(b)
    one = [[0, 12, 0, 0], [0, 19, 0, 0], [0, 8, 0, 0]]
    trio = [[0, 0, 12, 0], [0, 0, 19, 0], [0, 0, 8, 0]]
    assert b.taps == (trio if KVMUL_HS[case][1] == 96 else one), b.taps
    assert all(t[3] == 0 for t in b.taps)
    plan.freeTornadoExecutionPlan()


# ---- 2. one sequence's chunks (gl3_forward_prefill_seq)
@pytest.mark.parametrize("case", ["a", "b", "d", "h"], ids=["case_a", "case_b", "case_d", "case_h"])
def test_one_sequence_prefill(pkg, orc, planmod, case):
    """Chunks of 50 and 9 rows on a plan of batch 64, of 129 and 20 rows on a plan of batch 160 (the 129-row chunk of a and b leaves the
    one-launch kernel quantised for the wo GEMM: head size 128, more than 64 rows), then one forward whose logits are compared."""
    plan_mod, _ = planmod
    m = case_model(pkg, case, seed=62, ctx=160)
    for batch, chunks in ((64, [50, 9]), (160, [129, 20])):
        plan = plan_mod.HipMasterPlan(m, prefill_batch_size=batch, n_seqs=1)
        b = Mixed(orc, plan, [orc.COracle(m)], m, seed=8)
        for n in chunks:
            b.prefill(0, n)
            assert plan.attn_rows() == ([0, 0, n, 0] if KVMUL_HS[case][1] == 96 else [0, n, 0, 0]), (batch, n, plan.attn_rows())
        for p in (0, chunks[0] - 1, chunks[0], sum(chunks) - 1):      # layer 1's K / V rows come from layer 0's attention output
            k, v = plan.kv_seq(0, 1, p)
            ko, vo = b.oracles[0].kv(1, p)
            assert np.array_equal(k, ko) and np.array_equal(v, vo), (batch, p)
        b.step([(0, b.tokens(1))])
        plan.freeTornadoExecutionPlan()


# ---- 3. more than 64 rows in a mixed step
def test_more_than_64_rows(pkg, orc, planmod):
    """Case b at a context of 160, the row layout of test_gpu_mixed_batch.py::test_more_than_64_rows: a 70-row run, decode rows at depths 2, 9
    and 31, a 20-row run — 93 rows whose attention output leaves the grouped one-launch kernel quantised."""
    plan_mod, _ = planmod
    m = case_model(pkg, "b", seed=63, ctx=160)
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=128, n_seqs=5)
    b = Mixed(orc, plan, [orc.COracle(m) for _ in range(5)], m, seed=9)
    for seq, depth in ((1, 2), (2, 9), (3, 31)):
        b.prefill(seq, depth)
    b.step([(0, b.tokens(70)), (1, b.tokens(1)), (2, b.tokens(1)), (3, b.tokens(1)), (4, b.tokens(20))])
    assert b.pos == [70, 3, 10, 32, 20]
    assert plan.attn_rows() == [0, 93, 0, 0]
    plan.freeTornadoExecutionPlan()


# ---- 4. the split by depth: here with the shape's own limit, in a child pytest under GL3_PF_TAB_MAXPOS=40
@pytest.mark.parametrize("case", ["a", "d", "f"], ids=["case_a", "case_d", "case_f"])
def test_grouped_straddling_schedule(pkg, orc, planmod, case):
    """straddling_schedule of test_gpu_mixed_batch_depth.py (94 rows; under a limit of 40, 77 of them deep): the deep rows run the grouped
    table forms of pf_scores_mfma_kernel / pf_pv_mfma_kernel (under the VALU switches: pf_scores_pk_kernel<.., 4> / pf_pv_ring_kernel)."""
    plan_mod, _ = planmod
    m = case_model(pkg, case, seed=75, ctx=160)
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=128, n_seqs=5)
    b = Tapped(orc, plan, [orc.COracle(m) for _ in range(5)], m, seed=29, limit=limit_of(case))
    straddling_schedule(b)                       # (asserts [0, 17, 77, 0] itself under the limit of 40)
    assert b.taps == [expected_rows([(2, 1), (20, 70), (45, 1), (119, 21), (130, 1)], limit_of(case))]
    plan.freeTornadoExecutionPlan()


def test_the_split_under_a_lowered_limit():
    child({"GL3_PF_TAB_MAXPOS": "40"}, "test_grouped_straddling_schedule", 3)


# ---- 5. at real depth, no switch
def test_decode_row_at_560_beside_a_prompt_run(pkg, orc, planmod):
    """Case a at a context of 704, the layout of test_gpu_mixed_batch_depth.py::test_decode_row_at_560_beside_a_prompt_run: the limit of a
    grouped shape is that of kvMul 4 at its head size, position 511.  The 12-row run keeps the one-launch table form, the decode row at 560
    takes the trio; a one-sequence chunk that deep takes the trio (a grouped shape has no pf_attn_fused_kernel form, which is what carries
    kvMul 4 from position 512 to 639)."""
    plan_mod, _ = planmod
    m = case_model(pkg, "a", seed=65, ctx=704)
    assert limit_of("a") == 511
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=64, n_seqs=2)
    b = Tapped(orc, plan, [orc.COracle(m) for _ in range(2)], m, seed=11, limit=511)
    b.prefill(0, 560)
    b.step([(0, b.tokens(1)), (1, b.tokens(12))])
    assert b.pos == [561, 12] and b.taps == [[0, 12, 1, 0]]
    b.prefill(0, 64)                             # rows 561..624
    assert plan.attn_rows() == [0, 0, 64, 0]
    b.prefill(0, 36)                             # rows 625..660
    assert plan.attn_rows() == [0, 0, 36, 0]
    plan.freeTornadoExecutionPlan()


# ---- 6. value edges
def test_value_edges(pkg, orc, planmod):
    """edge_models' peaked-attn on case a through the three-step schedule: head 4 (first slot of kv head 0's ragged group) far out — softmax
    terms that are exactly 0 or f32-subnormal — heads 5 (its last real slot) and 6 (kv head 1) peaked less.  A surplus head slot that stored
    anything would overwrite a head of the next kv head or the next token's row."""
    plan_mod, _ = planmod
    m = em.make_edge_model("mid-qwen2", 8, 7, "peaked-attn")
    assert m.edits == ("peaked-attn",)
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=64, n_seqs=4)
    b = Tapped(orc, plan, [orc.COracle(m) for _ in range(4)], m, seed=19, limit=511)
    schedule(b)
    assert b.taps == [[0, 12, 0, 0], [0, 19, 0, 0], [0, 8, 0, 0]]
    plan.freeTornadoExecutionPlan()


# ---- 7. the VALU forms
def test_grouped_valu_forms():
    """GL3_PF_FUSED_MFMA=0 GL3_PF_SCORES_MFMA=0 GL3_PF_PV_MFMA=0 (read once per process): the schedule of test 1 on cases a and d runs the
    grouped pf_attn_fused2_kernel<128 | 64>; beside it, under a limit of 40, the straddling schedule on the same cases runs its deep rows on
    pf_scores_pk_kernel<.., 4> and pf_pv_ring_kernel.  Parity and no pair rows (the cases' own assertions)."""
    child({"GL3_PF_FUSED_MFMA": "0", "GL3_PF_SCORES_MFMA": "0", "GL3_PF_PV_MFMA": "0", "GL3_PF_TAB_MAXPOS": "40"},
          "(test_schedule_parity or test_grouped_straddling_schedule) and (case_a or case_d)", 4)


# ---- 8. unchanged paths
def test_single_row_steps_keep_their_dispatch(pkg, orc, planmod):
    """Case a, steps of single rows: attn_head_kernel while every row is below position 128, the per-row pair with a row past it — what
    test_gpu_mixed_batch_depth.py asserts for mid-llama."""
    plan_mod, _ = planmod
    m = case_model(pkg, "a", seed=67, ctx=200)
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=16, n_seqs=4)
    b = Mixed(orc, plan, [orc.COracle(m) for _ in range(4)], m, seed=13)
    for seq, n in enumerate((3, 126, 128, 130)):
        b.prefill(seq, n)
    b.step([(1, b.tokens(1)), (0, b.tokens(1))])                                    # positions 126 and 3
    assert plan.attn_rows() == [2, 0, 0, 0]
    b.step([(2, b.tokens(1)), (0, b.tokens(1)), (3, b.tokens(1)), (1, b.tokens(1))])        # 128, 4, 130, 127
    assert plan.attn_rows() == [0, 0, 0, 4]
    plan.freeTornadoExecutionPlan()
