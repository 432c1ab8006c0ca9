"""F16 on a 512-bit species (GL3_FLAG_VECTOR_512) through the batched paths: batched prefill, static-batched decode with the device
samplers, the attention hand-over at position 128 and the native host's --vector-bits switch.

FP16FloatTensor.vectorDot keeps 16 accumulator lanes on a 512-bit species; gemm_f16_mfma_v512_kernel (gl3_prefill_vl.h) runs that
order as sixteen f32-MFMA accumulator tiles shared by a wavefront pair.  Every comparison is np.array_equal on f32 against
COracle(m, vector_bits=512); where a silently dispatched 256-bit kernel could pass, the test also asserts that the 256-bit oracle
gives something else."""
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
from test_gpu_batch_decode_depth import MIXED_LENS, mixed_depth_schedule, model_with_ctx
from test_gpu_batch_sampling import SETTINGS, is_topp, mixed_generation
from test_gpu_run_host import EXE, llama_loop

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def planmod():
    from importlib import import_module
    ge.load_package()
    return import_module(ge.PKG_NAME + ".plan"), import_module(ge.PKG_NAME + ".hip")


@pytest.mark.parametrize("cfg,batch,chunks", [("mid-llama", 64, [40, 23, 3]),
                                              ("mid-qwen3", 32, [30, 7]),               # per-head norm, head size 128
                                              ("mid-qwen2", 16, [16, 5]),               # bias
                                              ("mid-phi3", 64, [64, 1]),                # fused tensors, exact tile
                                              ("mid-granite", 64, [35, 2]),             # scalars
                                              ("tiny-llama-tied", 128, [70, 9])])       # second 64-token tile, ragged, behind a non-zero start
def test_batched_prefill_of_f16_on_a_512_bit_species(pkg, orc, planmod, cfg, batch, chunks):
    """x of the last token after every chunk, KV rows, the two decode steps that follow; the chunk's X rows are in the batched buffer
    (a plan without batched state has none: the chunk did not run token by token); the 256-bit order gives something else.
    tiny-llama-tied has 48 positions: its case gets the context its 79 + 2 tokens need, everything else of the config stays."""
    plan_mod, hip = planmod
    m = model_with_ctx(pkg, cfg, max(pkg.synth.CONFIGS[cfg].ctx, sum(chunks) + 2), seed=35, wtype=1)
    plan = plan_mod.HipMasterPlan.initializeTornadoVMPlan(m, prefill_batch_size=batch, flags=hip.FLAG_VECTOR_512)
    o, o256 = orc.COracle(m, vector_bits=512), orc.COracle(m, vector_bits=256)
    n, dim = sum(chunks), m.cfg.dim
    toks = pkg.javarand.bench_tokens(m.cfg.vocab, n + 2)
    pos, differs = 0, False
    for c in chunks:
        plan.tornadoVMForwardBatchPrefill(toks[pos:pos + c], pos)
        o.prefill(toks[pos:pos + c], pos); o256.prefill(toks[pos:pos + c], pos)
        pos += c
        x = plan.x()
        assert np.array_equal(x, o.x()), pos
        differs |= not np.array_equal(x, o256.x())
        rows = plan.buffer(4, c * dim).reshape(c, dim)
        assert np.array_equal(rows[c - 1], x), pos
    for l in range(m.cfg.n_layers):
        for p in (0, 1, n // 2, n - 1):
            k, v = plan.kv(l, p)
            ko, vo = o.kv(l, p)
            assert np.array_equal(k, ko) and np.array_equal(v, vo), (l, p)
    for i in range(2):
        got = plan.tornadoVMForwardDecode(toks[n + i], n + i)
        assert np.array_equal(got, o.forward(toks[n + i], n + i)), i
        differs |= not np.array_equal(got, o256.forward(toks[n + i], n + i))
    assert differs, "the 256-bit order passes the same checks"
    plan.freeTornadoExecutionPlan()


@pytest.mark.parametrize("cfg,nseq", [("mid-llama", 3), ("mid-qwen3", 5), ("tiny-llama-tied", 17)])
def test_static_batched_decode_of_f16_on_a_512_bit_species(pkg, orc, planmod, cfg, nseq):
    """n sequences with prompts of different lengths advance one token per step; logits and greedy id of every row equal that
    sequence's own oracle run, and so does the KV row each step wrote."""
    plan_mod, hip = planmod
    m = pkg.synth.make_numpy(pkg.synth.CONFIGS[cfg], wtype=1, seed=45)
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=max(16, nseq), n_seqs=nseq, flags=hip.FLAG_VECTOR_512)
    oracles = [orc.COracle(m, vector_bits=512) for _ in range(nseq)]
    o256 = orc.COracle(m, vector_bits=256)                      # shadows sequence 0
    rng = np.random.default_rng(5)
    lens = [2 + (i % 4) for i in range(nseq)]
    for s_ in range(nseq):
        prompt = rng.integers(0, m.cfg.vocab, lens[s_]).tolist()
        plan.prefill_seq(s_, prompt, 0)
        oracles[s_].prefill(prompt, 0)
        if s_ == 0:
            o256.prefill(prompt, 0)
    cur = [int(rng.integers(0, m.cfg.vocab)) for _ in range(nseq)]
    pos = list(lens)
    differs = False
    for step in range(3):
        order = list(range(nseq))
        if step % 2:
            order.reverse()
        logits, ids = plan.forward_decode_batch([cur[s_] for s_ in order], order, [pos[s_] for s_ in order])
        for row, s_ in enumerate(order):
            ref = oracles[s_].forward(cur[s_], pos[s_])
            assert np.array_equal(logits[row], ref), (step, s_)
            assert ids[row] == orc.argmax(ref)
            if s_ == 0:
                differs |= not np.array_equal(ref, o256.forward(cur[s_], pos[s_]))
            cur[s_], pos[s_] = int(ids[row]), pos[s_] + 1
    assert differs, "the 256-bit order passes the same checks"
    for s_ in range(nseq):
        for l in range(m.cfg.n_layers):
            k, v = plan.kv_seq(s_, l, pos[s_] - 1)              # the row the last step wrote
            ko, vo = oracles[s_].kv(l, pos[s_] - 1)
            assert np.array_equal(k, ko) and np.array_equal(v, vo), (s_, l)
    plan.freeTornadoExecutionPlan()


def test_batched_samplers_behind_the_512_bit_gemm(pkg, orc, planmod):
    """One sampled step of 4 rows: top-p, categorical, greedy and top-p again (SETTINGS[0..3]), coins from the caller; ids and the
    probabilities they were drawn from equal the oracle's sampler on the 512-bit oracle's logits."""
    plan_mod, hip = planmod
    nseq = 4
    assert [is_topp(*s) for s in SETTINGS[:nseq]] == [True, False, False, True] and SETTINGS[2][0] == 0 and SETTINGS[1][0] > 0
    m = pkg.synth.make_numpy(pkg.synth.CONFIGS["mid-llama"], wtype=1, seed=83)
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=16, n_seqs=nseq, flags=hip.FLAG_VECTOR_512)
    oracles = [orc.COracle(m, vector_bits=512) for _ in range(nseq)]
    _, pos, n_topp = mixed_generation(pkg, orc, plan, oracles, m, nseq, 1)
    assert n_topp == 2 and sum(plan.topp_counts()) == n_topp and pos == [4, 6, 8, 10]
    plan.freeTornadoExecutionPlan()


def test_handover_at_128_of_f16_on_a_512_bit_species(pkg, orc, planmod):
    """The schedule of test_handover_at_128_of_the_f32_activation_types (captured and eager steps, rows crossing 127 -> 128, prompts of
    more than 64 tokens into sequences other than 0) on a plan of the 512-bit species."""
    plan_mod, hip = planmod
    m = model_with_ctx(pkg, "mid-llama", 200, seed=53, wtype=1)
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=160, n_seqs=len(MIXED_LENS), flags=hip.FLAG_VECTOR_512)
    oracles = [orc.COracle(m, vector_bits=512) for _ in MIXED_LENS]
    mixed_depth_schedule(orc, plan, oracles, m, seed=17)
    plan.freeTornadoExecutionPlan()


def test_native_host_selects_the_species(pkg, orc, tmp_path):
    """gl3_run --vector-bits 512 -b 16 on an F16 GGUF generates the ids of the 512-bit oracle's greedy run.  Greedy ids survive a change
    of the summation order on these small models, so the proof that the switch reaches the plan is the refusal it earns on a Q4_0 file
    (Q4_0FloatTensor.vectorDot throws on a 512-bit species; 256 is accepted there); any other width is a usage error."""
    m = pkg.synth.make_numpy(pkg.synth.CONFIGS["tiny-llama"], wtype=1, seed=31)
    path = str(tmp_path / "m.gguf")
    m.write_gguf(path)
    prompt = pkg.javarand.bench_tokens(m.cfg.vocab, 21)         # begin-of-text + 21 ids: a full chunk of 16 and a ragged one
    want = llama_loop(orc, orc.COracle(pkg.synth.SynthModel.from_gguf(path), vector_bits=512), prompt, 1, 40, set(), orc.argmax)

    def run(model, bits, n):
        return subprocess.run([EXE, "-m", model, "--ids", ",".join(map(str, prompt)), "-n", str(n), "-b", "16", "--bos", "1", "--vector-bits", bits],
                              capture_output=True, text=True, timeout=180)
    out = run(path, "512", 40)
    assert out.returncode == 0, out.stderr
    assert [int(x) for x in out.stdout.split("generated:")[1].split()] == want and len(want) > 8
    bad = run(path, "384", 40)
    assert bad.returncode == 2 and "--vector-bits" in bad.stderr
    q4 = str(tmp_path / "q4.gguf")
    pkg.synth.make_numpy(pkg.synth.CONFIGS["tiny-llama-tied"], wtype=2, seed=3).write_gguf(q4)
    refused = run(q4, "512", 24)
    assert refused.returncode == 1 and "(-2)" in refused.stderr, refused.stderr
    assert run(q4, "256", 24).returncode == 0
