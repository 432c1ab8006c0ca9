"""Static-batched decode (gl3_forward_decode_batch) past position 127 and at mixed depths, bit for bit against one CPU oracle per sequence.

From the first step in which any row sits at position >= 128 (AF_MAXN) the step is a different program: the one-launch attention
(attn_head_kernel) gives way to pf_rope_kv_kernel + pf_attn_scores_kernel + pf_attn_softmax_pv_kernel, which read every row's
sequence id and position from device memory on a grid sized by the DEEPEST row; the attention output reaches the wo GEMM through
the separate quantise launch while gate + up / down stay on the fused-quantised hand-over; the step is enqueued eagerly instead of
replayed from its captured graph (a batch that mixes depths flips between the two from step to step); and rows longer than the
softmax window run windowed.  The tests below drive each of these with per-row differing sequences and positions, every batch
tile class (1 .. 96 rows: the 32- and 64-slot operand layouts, every 16-token tile edge, the chunk-major GEMMs above 64 rows),
prefill chunks of more than 64 tokens into sequences other than 0, the f32-activation weight types and the batched sampler.

Every comparison is np.array_equal on f32: logits and greedy id of every row of every step, and after the last step the K / V
rows of every layer at every position a batched step wrote, one position before the first such write and one after the last (a
write that lands in another sequence's cache or on another row shows up there).  tests/test_gpu_gemm_forms.py runs this file
again under GL3_NO_FUSED_BD_ATTN / GL3_NO_FUSED_QUANT, where the three-kernel attention also serves the shallow rows."""
import numpy as np
import pytest

import __graft_entry__ as ge
# pytest reuses this module object for tests/test_gpu_batch_sampling.py itself, so its global DRAWS tally is shared: call nothing here that
# counts into it (count_draws), or that file's device-share check would see this file's draws
from test_gpu_batch_sampling import mixed_generation

pytestmark = pytest.mark.gpu
AF_MAXN = 128          # gl3_decode_kernels.h: positions below it take the one-launch attention and the captured step


@pytest.fixture(scope="module")
def planmod():
    from importlib import import_module
    ge.load_package()
    return import_module(ge.PKG_NAME + ".plan"), import_module(ge.PKG_NAME + ".hip")


def model_with_ctx(pkg, cfg, ctx, seed, wtype=8):
    base = pkg.synth.CONFIGS[cfg]
    return pkg.synth.make_numpy(pkg.synth.ModelConfig(**{**base.__dict__, "ctx": ctx}), wtype=wtype, seed=seed)


class Batch:
    """n sequences on a plan and on one oracle each: prefill both sides, run batched steps, compare."""

    def __init__(self, orc, plan, oracles, m, lens, seed, calls=None):
        """lens[s]: prompt length of sequence s; calls[s] (optional): the prompt enters in prefill_seq calls of these sizes (each call is
        cut into chunks of the plan's max_batch)."""
        self.orc, self.plan, self.oracles, self.m = orc, plan, oracles, m
        rng = np.random.default_rng(seed)
        for s, n in enumerate(lens):
            prompt = rng.integers(0, m.cfg.vocab, n).tolist()
            off = 0
            for c in (calls or {}).get(s, [n]):
                plan.prefill_seq(s, prompt[off:off + c], off)
                off += c
            assert off == n
            oracles[s].prefill(prompt, 0)
        self.cur = [int(rng.integers(0, m.cfg.vocab)) for _ in lens]
        self.pos = list(lens)
        self.first = {}                      # sequence -> position of its first batched step
        self.log = []                        # per step: (row order, positions of the rows)

    def step(self, order):
        cur, pos = self.cur, self.pos
        at = [pos[s] for s in order]
        logits, ids = self.plan.forward_decode_batch([cur[s] for s in order], order, at)
        self.log.append((list(order), at))
        for row, s in enumerate(order):
            ref = self.oracles[s].forward(cur[s], pos[s])
            assert np.array_equal(logits[row], ref), ("logits", len(self.log) - 1, "row", row, "seq", s, "pos", pos[s], "rows", len(order))
            assert int(ids[row]) == self.orc.argmax(ref), ("id", len(self.log) - 1, "row", row, "seq", s, "pos", pos[s])
            self.first.setdefault(s, pos[s])
            cur[s], pos[s] = int(ids[row]), pos[s] + 1          # greedy continuation per sequence

    def check_kv(self):
        """Every position a batched step wrote, one before the first and one after the last.  The position after the last has been written by
        nobody: the plan and the oracle both start from a zeroed cache, so anything but zeros there is a stray write."""
        ctx = self.m.cfg.ctx
        checked = 0
        for s, first in sorted(self.first.items()):
            for l in range(self.m.cfg.n_layers):
                for p in range(max(first - 1, 0), min(self.pos[s], ctx - 1) + 1):      # pos[s] - 1 is the last row a step wrote
                    k, v = self.plan.kv_seq(s, l, p)
                    ko, vo = self.oracles[s].kv(l, p)
                    assert np.array_equal(k, ko) and np.array_equal(v, vo), ("kv", "seq", s, "layer", l, "pos", p)
                    checked += 1
        assert checked > 0


def rotated(members, step):
    k = step % len(members)
    order = members[k:] + members[:k]
    return order[::-1] if (step // 2) % 2 else order


MIXED_LENS = [124, 3, 127, 60, 131]
MIXED_CALLS = {0: [70, 54]}                  # sequences 2 and 4 enter in one chunk of > 64 tokens each (prefill_batch_size 160)


def mixed_depth_schedule(orc, plan, oracles, m, seed, steps=10):
    """Even steps: the full batch (sequence 4 is beyond 128 from the start: eager launches, three-kernel attention, shallow rows leave the
    deep row's grid early).  Odd steps: the sequences still below 128 (captured step, straight after an eager one).  Sequences 0 and 2
    walk 127 -> 128 during the run."""
    b = Batch(orc, plan, oracles, m, MIXED_LENS, seed, MIXED_CALLS)
    for step in range(steps):
        members = list(range(len(MIXED_LENS))) if step % 2 == 0 else [s for s in range(len(MIXED_LENS)) if b.pos[s] < AF_MAXN]
        b.step(rotated(members, step))
    # the schedule is what the docstring says (a later edit of the lengths must not turn this into a shallow test)
    eager = [max(at) >= AF_MAXN for _, at in b.log]
    assert len(b.log) >= 9 and any(eager) and not all(eager)
    assert any(eager[i] and not eager[i + 1] for i in range(len(eager) - 1)), "no captured step straight after an eager one"
    assert any(e and min(at) < 64 and max(at) >= AF_MAXN for e, (_, at) in zip(eager, b.log)), "no eager step with a row that leaves the deep grid early"
    assert all(b.log[i][0] != b.log[i + 1][0] for i in range(len(b.log) - 1))
    full = [tuple(o) for o, _ in b.log if len(o) == len(MIXED_LENS)]
    assert len(set(full)) == len(full) >= 5, "full-batch steps must all differ in row order"
    for s in (0, 2):
        seen = [at[o.index(s)] for o, at in b.log if s in o]
        assert AF_MAXN - 1 in seen and AF_MAXN in seen, ("sequence does not cross 127 -> 128", s, seen)
    assert any(AF_MAXN - 1 in at and not e for e, (_, at) in zip(eager, b.log)), "no captured step with a row at the last fused position"
    b.check_kv()


@pytest.mark.parametrize("cfg", ["mid-llama", "mid-qwen3", "mid-qwen2", "mha-llama", "mid-granite", "phi3-hs96", "mid-devstral"])
def test_handover_at_128_with_mixed_depths(pkg, orc, planmod, cfg):
    """Head sizes 64 / 128 / 96, kvMul 4 / 6 / 1, qk-norm, bias, attention scale.  The 131- and 127-token prompts enter sequences 4 and 2
    as one chunk of more than 64 tokens each (chunk-major GEMMs and, for head size 128, the quantised attention output, at a non-zero
    sequence offset of the caches); the 124-token prompt in calls of 70 and 54 tokens."""
    plan_mod, _ = planmod
    m = model_with_ctx(pkg, cfg, 200, seed=51)
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=160, n_seqs=len(MIXED_LENS))
    oracles = [orc.COracle(m) for _ in MIXED_LENS]
    mixed_depth_schedule(orc, plan, oracles, m, seed=13)
    plan.freeTornadoExecutionPlan()


@pytest.mark.parametrize("cfg,wtype,f32act", [("mid-llama", 1, False), ("mid-llama", 2, False), ("mid-qwen3", 8, True)])
def test_handover_at_128_of_the_f32_activation_types(pkg, orc, planmod, cfg, wtype, f32act):
    """F16 / Q4_0 / Q8_0 with the f32 activation (pf_layers_vl: Vector-API-order GEMMs around the same attention kernels)."""
    plan_mod, hip = planmod
    m = model_with_ctx(pkg, cfg, 200, seed=53, wtype=wtype)
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=160, n_seqs=len(MIXED_LENS), flags=hip.FLAG_F32_ACTIVATION if f32act else 0)
    oracles = [orc.COracle(m, vector_bits=256, f32_activation=f32act) for _ in MIXED_LENS]
    mixed_depth_schedule(orc, plan, oracles, m, seed=17)
    plan.freeTornadoExecutionPlan()


ROW_COUNTS = [1, 16, 17, 32, 33, 64, 65, 96]      # 32- and 64-slot operand layouts, every 16-token tile edge, > 64 rows: chunk-major GEMMs
N_TILE_SEQS = 96


def tile_class_steps(b):
    for k, n in enumerate(ROW_COUNTS):
        order = [(7 * k + 5 * i) % N_TILE_SEQS for i in range(n)]      # 5 is coprime to 96: n distinct sequences, row != sequence id
        assert len(set(order)) == n
        b.step(order)
    assert sorted(b.first) == list(range(N_TILE_SEQS))


@pytest.mark.parametrize("cfg", ["tiny-llama", "tiny-qwen3"])      # head sizes 32 / 64
def test_every_batch_tile_class_beyond_128_positions(pkg, orc, planmod, cfg):
    plan_mod, _ = planmod
    m = model_with_ctx(pkg, cfg, 160, seed=55)
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=N_TILE_SEQS, n_seqs=N_TILE_SEQS)
    oracles = [orc.COracle(m) for _ in range(N_TILE_SEQS)]
    b = Batch(orc, plan, oracles, m, [AF_MAXN + (11 * s) % 6 for s in range(N_TILE_SEQS)], seed=19)      # 128 .. 133 positions
    assert {min(b.pos), max(b.pos)} == {AF_MAXN, AF_MAXN + 5}
    tile_class_steps(b)
    assert all(min(at) >= AF_MAXN for _, at in b.log)
    b.check_kv()
    plan.freeTornadoExecutionPlan()


@pytest.mark.parametrize("cfg", ["tiny-llama", "tiny-qwen3"])
def test_every_batch_tile_class_at_shallow_positions(pkg, orc, planmod, cfg):
    """The same row counts on the one-launch attention and the captured steps: 65 and 96 rows there run the chunk-major GEMMs with the
    separate quantise launches."""
    plan_mod, _ = planmod
    m = model_with_ctx(pkg, cfg, 160, seed=55)
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=N_TILE_SEQS, n_seqs=N_TILE_SEQS)
    oracles = [orc.COracle(m) for _ in range(N_TILE_SEQS)]
    b = Batch(orc, plan, oracles, m, [1 + (7 * s) % 5 for s in range(N_TILE_SEQS)], seed=23)             # 1 .. 5 positions
    tile_class_steps(b)
    assert all(max(at) < AF_MAXN for _, at in b.log)
    b.check_kv()
    plan.freeTornadoExecutionPlan()


@pytest.mark.parametrize("cfg", ["tiny-llama", "phi3-hs96"])
def test_windowed_softmax_rows_in_a_batched_step(pkg, orc, planmod, cfg, monkeypatch):
    """GL3_ATTN_WINDOW = 1024 (read in gl3_create): sequence 0's rows (1101 .. 1104 scores) run in two windows with the sequential sum
    carried across, sequence 1's row length passes the window edge during the run (1023, 1024, 1025, 1026), sequence 2 is shallow —
    all in one launch, in changing row order."""
    plan_mod, _ = planmod
    window = 1024
    monkeypatch.setenv("GL3_ATTN_WINDOW", str(window))
    m = model_with_ctx(pkg, cfg, 1300, seed=57)
    lens = [1100, 1022, 5]
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=512, n_seqs=len(lens))
    oracles = [orc.COracle(m) for _ in lens]
    b = Batch(orc, plan, oracles, m, lens, seed=29)
    for order in ([0, 1, 2], [2, 1, 0], [1, 2, 0], [2, 0, 1]):
        b.step(order)
    rows1 = [at[o.index(1)] + 1 for o, at in b.log]           # softmax row lengths of sequence 1
    assert min(rows1) < window and window in rows1 and max(rows1) > window
    assert all(at[o.index(0)] + 1 > window for o, at in b.log)
    b.check_kv()
    plan.freeTornadoExecutionPlan()


@pytest.mark.parametrize("lens", [[126, 3, 131, 60], [125, 3, 126, 60]], ids=["deep-row-from-the-start", "captured-then-eager"])
def test_batched_sampler_behind_an_eager_step(pkg, orc, planmod, lens):
    """forward_decode_batch_sample at mixed depths across 128, with the settings table and the coin stream of test_gpu_batch_sampling.py:
    sampled ids and the probabilities they were drawn from equal the oracle's sampler on the oracle's logits.  First case: every step is
    eager, sequence 0 crosses 127 -> 128.  Second case: two captured steps (deepest row at 126, 127), then eager ones."""
    plan_mod, _ = planmod
    nseq, steps = len(lens), 5
    m = model_with_ctx(pkg, "mid-llama", 200, seed=83)
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=160, n_seqs=nseq)
    oracles = [orc.COracle(m) for _ in range(nseq)]
    cur, pos, n_topp = mixed_generation(pkg, orc, plan, oracles, m, nseq, steps, lens=lens)
    assert pos == [n + steps for n in lens] and max(lens) + steps > AF_MAXN > min(lens) + steps
    assert any(n <= AF_MAXN - 1 and n + steps - 1 >= AF_MAXN for n in lens), "no sequence crosses 127 -> 128"
    assert n_topp > 0 and sum(plan.topp_counts()) == n_topp
    for s in range(nseq):                                     # the sampled steps wrote the right KV rows of the right sequences
        for l in range(m.cfg.n_layers):
            for p in range(lens[s] - 1, pos[s] + 1):
                k, v = plan.kv_seq(s, l, p)
                ko, vo = oracles[s].kv(l, p)
                assert np.array_equal(k, ko) and np.array_equal(v, vo), (s, l, p)
    plan.freeTornadoExecutionPlan()
