"""Parity on edge VALUES: the models of tests/edge_models.py (zero / f16-subnormal / rounds-to-zero / outlier activation blocks, zero,
subnormal, negative and large block scales, -128 and +-127 quants with block dots at their bound, f16 subnormals / +-0 / 65504 in whole
lane groups, peaked attention with exp terms that are 0 or f32-subnormal, ties, a router with one full and many empty experts) through
every path the suite otherwise runs on randn * 0.02 only.  tests/test_edge_models.py shows on the CPU that the models reach those
conditions.  Everything is np.array_equal on f32 against COracle computed at run time: logits, x behind every layer, K / V rows."""
import os
import subprocess
import sys

import numpy as np
import pytest

import __graft_entry__ as ge
import edge_models as em
from test_gpu_batch_decode_depth import Batch
from test_gpu_mixed_batch import Mixed
from test_gpu_moe_batched import compare_kv, prefill_chunk_and_compare

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(__file__), "golden")
Q8_EDITS = list(em.edits_for(8, 0, "all")) + ["all"]


@pytest.fixture(scope="module")
def planmod():
    from importlib import import_module
    ge.load_package()
    return import_module(ge.PKG_NAME + ".plan"), import_module(ge.PKG_NAME + ".hip")


def finite(ref):
    assert np.all(np.isfinite(ref)), "the test MODEL leaves the finite range (NaN / Inf are out of scope): fix edge_models.py"
    return ref


def decode_and_compare(plans, o, toks, start=0, taps=True):
    """Decode steps toks[start:] on every plan against oracle o: logits, layer taps, and at the end the K / V rows of every position."""
    n_layers = plans[0].cfg.n_layers
    for pos in range(start, len(toks)):
        ref, lx = o.forward(toks[pos], pos, layer_x=True)
        finite(ref)
        for i, plan in enumerate(plans):
            got = plan.tornadoVMForwardDecode(toks[pos], pos)
            if taps:
                for l in range(n_layers):
                    assert np.array_equal(plan.layer_x(l), lx[l]), ("layer_x", "plan", i, "pos", pos, "layer", l)
            assert np.array_equal(got, ref), ("logits", "plan", i, "pos", pos)
    for plan in plans:
        for l in range(n_layers):
            for pos in range(len(toks)):
                k, v = plan.kv(l, pos)
                ko, vo = o.kv(l, pos)
                assert np.array_equal(k, ko) and np.array_equal(v, vo), ("kv", l, pos)


def prefill_chunks(plan, o, toks, chunks):
    pos = 0
    for c in chunks:
        plan.tornadoVMForwardBatchPrefill(toks[pos:pos + c], pos)
        o.prefill(toks[pos:pos + c], pos)
        pos += c
        assert np.array_equal(plan.x(), finite(o.x())), ("x behind chunk", pos)
    return pos


# ---- 1: Q8_0 decode, graph replay and eager
CASE1 = [("tiny-llama", e) for e in Q8_EDITS] + [("tiny-llama-kv4", "all"), ("tiny-qwen3", "all"), ("tiny-qwen3", "act-blocks"), ("tiny-qwen2", "all"),
                                                   ("tiny-granite", "all"), ("tiny-phi3", "all"), ("tiny-phi3", "inner-act-blocks")]


def edge_model(cfg, wtype, edits, **over):
    if cfg == "tiny-llama-kv4":                 # four 32-row groups of V: the only llama shape with an f16-subnormal block INTO wo
        return em.make_edge_model("tiny-llama", wtype, 7, edits, n_kv_heads=4, **over)
    return em.make_edge_model(cfg, wtype, 7, edits, **over)


@pytest.mark.parametrize("cfg,edits", CASE1, ids=["%s-%s" % c for c in CASE1])
def test_q8_0_decode_graph_and_eager(pkg, orc, planmod, cfg, edits):
    plan_mod, hip = planmod
    m = edge_model(cfg, 8, edits)
    plans = [plan_mod.HipMasterPlan(m, flags=hip.FLAG_LAYER_TAPS), plan_mod.HipMasterPlan(m, flags=hip.FLAG_LAYER_TAPS | hip.FLAG_NO_GRAPH)]
    decode_and_compare(plans, orc.COracle(m), em.edge_tokens(pkg, m, 12))
    [p.freeTornadoExecutionPlan() for p in plans]


# ---- 2: the committed fixture
def test_decode_matches_the_edge_fixture(pkg, planmod):
    plan_mod, hip = planmod
    g = np.load(os.path.join(GOLD, "tiny_llama_q8_0_edges.npz"))
    m = em.make_edge_model("tiny-llama", 8, 7, "all")
    plan = plan_mod.HipMasterPlan(m, flags=hip.FLAG_LAYER_TAPS)
    toks = g["tokens"]
    n_prompt, steps = len(g["prompt"]), g["logits"].shape[0]
    for pos in range(steps):
        lg = plan.tornadoVMForwardDecode(int(toks[pos]), pos)
        assert np.array_equal(lg, g["logits"][pos]), pos
        if pos >= n_prompt - 1:
            assert int(np.argmax(lg)) == toks[pos + 1], pos
    for l in range(m.cfg.n_layers):
        assert np.array_equal(plan.layer_x(l), g["last_layer_x"][l])
        k, v = plan.kv(l, steps - 1)
        assert np.array_equal(k, g["k_last"][l]) and np.array_equal(v, g["v_last"][l])
    plan.freeTornadoExecutionPlan()


# ---- 3: the other weight types
def modes(hip):
    return {"f16-scalar": (1, hip.FLAG_SCALAR_DOT, dict(vector_bits=0)), "f16-v256": (1, 0, dict(vector_bits=256)),
            "f16-v512": (1, hip.FLAG_VECTOR_512, dict(vector_bits=512)), "q4_0-scalar": (2, hip.FLAG_SCALAR_DOT, dict(vector_bits=0)),
            "q4_0-v256": (2, 0, dict(vector_bits=256)), "q8_0-f32act": (8, hip.FLAG_F32_ACTIVATION, dict(vector_bits=256, f32_activation=True))}


@pytest.mark.parametrize("cfg", ["tiny-llama", "tiny-llama-tied"])
@pytest.mark.parametrize("mode", ["f16-scalar", "f16-v256", "f16-v512", "q4_0-scalar", "q4_0-v256", "q8_0-f32act"])
def test_other_weight_types(pkg, orc, planmod, cfg, mode):
    """Decode from position 0, one batched prefill [37, 20] with two decode steps behind it, one static-batched step of 5 rows (the scalar
    order has no batched paths: its prefill runs token by token and the batched step is refused)."""
    plan_mod, hip = planmod
    wt, flags, okw = modes(hip)[mode]
    m = em.make_edge_model(cfg, wt, 7, "all", ctx=64)
    toks = em.edge_tokens(pkg, m, 59)
    plan = plan_mod.HipMasterPlan(m, flags=flags | hip.FLAG_LAYER_TAPS)
    decode_and_compare([plan], orc.COracle(m, **okw), toks[:12])
    plan.freeTornadoExecutionPlan()
    plan = plan_mod.HipMasterPlan.initializeTornadoVMPlan(m, prefill_batch_size=64, flags=flags | hip.FLAG_LAYER_TAPS)
    o = orc.COracle(m, **okw)
    if flags & hip.FLAG_SCALAR_DOT:
        plan.prefill(toks[:57], 0)
        o.prefill(toks[:57], 0)
    else:
        prefill_chunks(plan, o, toks, [37, 20])
    decode_and_compare([plan], o, toks, start=57)
    plan.freeTornadoExecutionPlan()
    if flags & hip.FLAG_SCALAR_DOT:
        return
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=16, n_seqs=5, flags=flags)
    b = Batch(orc, plan, [orc.COracle(m, **okw) for _ in range(5)], m, [2, 3, 4, 5, 2], seed=5)
    b.cur[1], b.cur[3] = em.ZERO_TOKEN, em.FLAT_TOKEN
    b.step([3, 0, 4, 1, 2])
    b.check_kv()
    plan.freeTornadoExecutionPlan()


# ---- 4 / 5: attention regimes
ATTN = [("tiny-llama", ("act-blocks", "peaked-attn")), ("tiny-qwen3", ("act-blocks", "peaked-attn")), ("tiny-llama", "all"), ("tiny-qwen3", "all")]


@pytest.mark.parametrize("cfg,edits", ATTN, ids=["%s-%s" % (c, e if isinstance(e, str) else "+".join(e)) for c, e in ATTN])
def test_decode_attention_regimes_behind_batched_prefill(pkg, orc, planmod, cfg, edits):
    """Batched prefill to 120 / 130 / 770 positions (the one-launch prefill attention, K = 1 f32 MFMA products), then two decode steps each:
    attn_head_kernel below 128, attn_scores + attn_softmax_pv below 768, the four-launch path from 768 on."""
    plan_mod, hip = planmod
    m = em.make_edge_model(cfg, 8, 7, edits, ctx=832)
    plan = plan_mod.HipMasterPlan.initializeTornadoVMPlan(m, prefill_batch_size=256)
    o = orc.COracle(m)
    toks = em.edge_tokens(pkg, m, 780)
    for p in (300, 301, 600):                          # the zero-embedding token deep in the context as well
        toks[p] = em.ZERO_TOKEN
    done = 0
    for depth in (120, 130, 770):
        while done < depth:
            c = min(256, depth - done)
            plan.tornadoVMForwardBatchPrefill(toks[done:done + c], done)
            o.prefill(toks[done:done + c], done)
            done += c
        for pos in range(depth, depth + 2):
            ref = finite(o.forward(toks[pos], pos))
            assert np.array_equal(plan.forward_decode(toks[pos], pos), ref), (cfg, pos)
            done = pos + 1
        for l in range(m.cfg.n_layers):
            for p in (0, 2, depth - 1, done - 1):
                k, v = plan.kv(l, p)
                ko, vo = o.kv(l, p)
                assert np.array_equal(k, ko) and np.array_equal(v, vo), (cfg, l, p)
    plan.freeTornadoExecutionPlan()


@pytest.mark.parametrize("cfg,edits", ATTN, ids=["%s-%s" % (c, e if isinstance(e, str) else "+".join(e)) for c, e in ATTN])
def test_static_batched_step_with_rows_on_both_sides_of_128(pkg, orc, planmod, cfg, edits):
    plan_mod, hip = planmod
    m = em.make_edge_model(cfg, 8, 7, edits, ctx=200)
    lens = [126, 3, 131, 60]
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=160, n_seqs=len(lens))
    b = Batch(orc, plan, [orc.COracle(m) for _ in lens], m, lens, seed=23)
    b.cur[0] = em.ZERO_TOKEN
    for step in range(3):                              # sequence 0 walks 126 -> 128; the last step is the shallow rows alone (captured step)
        b.step([2, 0, 3, 1] if step < 2 else [1, 3])
    b.check_kv()
    plan.freeTornadoExecutionPlan()


# ---- 6 / 7: batched prefill
@pytest.mark.parametrize("cfg,edits", [("tiny-llama", "all"), ("tiny-llama-kv4", "all"), ("tiny-qwen3", "all"), ("tiny-phi3", "all"), ("tiny-llama", "act-blocks"),
                                       ("tiny-llama", "w-scales"), ("tiny-llama", "w-quants")])
def test_batched_prefill_up_to_64_tokens(pkg, orc, planmod, cfg, edits):
    """bdw_gemm_kernel and the fused quantiser: chunks [37, 20], then two decode steps."""
    plan_mod, hip = planmod
    m = edge_model(cfg, 8, edits)
    plan = plan_mod.HipMasterPlan.initializeTornadoVMPlan(m, prefill_batch_size=64, flags=hip.FLAG_LAYER_TAPS)
    o = orc.COracle(m)
    toks = em.edge_tokens(pkg, m, 59)
    prefill_chunks(plan, o, toks, [37, 20])
    decode_and_compare([plan], o, toks, start=57)
    plan.freeTornadoExecutionPlan()


@pytest.mark.parametrize("cfg,edits", [("ragged-llama", "all"), ("tiny-devstral", "all"), ("ragged-llama", "act-blocks"), ("ragged-llama", "w-scales"),
                                       ("ragged-llama", "inner-act-blocks")])
def test_batched_prefill_above_64_tokens(pkg, orc, planmod, cfg, edits):
    """pf_gemm3_kernel, the tall gate / up form that writes hb quantised, pf_attn_fused3_kernel that writes xb quantised: chunks [70, 65].
    ragged-llama: K = 9 / 27 blocks, the edge blocks of ffn_norm / output_norm and of w-scales sit in the last real K block, next to the
    zero scale operands of the padded ones."""
    plan_mod, hip = planmod
    m = em.make_edge_model(cfg, 8, 7, edits, ctx=200)
    plan = plan_mod.HipMasterPlan.initializeTornadoVMPlan(m, prefill_batch_size=70, flags=hip.FLAG_LAYER_TAPS)
    o = orc.COracle(m)
    toks = em.edge_tokens(pkg, m, 137)
    toks[80] = toks[134] = em.ZERO_TOKEN
    prefill_chunks(plan, o, toks, [70, 65])
    decode_and_compare([plan], o, toks, start=135)
    plan.freeTornadoExecutionPlan()


# ---- 8: the forms, each in its own process (the library reads its switches once)
PREFILL = "(above_64_tokens or attention_regimes) and all"       # cases 7 and 4 on the "all" models: 4 tests
BATCHED = "(above_64_tokens or both_sides_of_128) and all"        # cases 7 and 5: 4 tests
FORMS = [({"GL3_PF_GEMM3_TALL": "-1"}, PREFILL), ({"GL3_PF_GEMM3_TALL": "4"}, PREFILL), ({"GL3_PF_GEMM3_TALL": "5", "GL3_PF_GEMM3_TALL_KB": "1"}, PREFILL),
         ({"GL3_PF_GEMM3_TALL": "7", "GL3_PF_GEMM3_SHAPE": "1"}, PREFILL), ({"GL3_PF_GEMM3_TALL": "6", "GL3_PF_GEMM3_SHAPE": "2"}, PREFILL),
         ({"GL3_PF_FUSED_ATTN": "0"}, PREFILL),
         ({"GL3_PF_FUSED_ATTN": "0", "GL3_PF_SCORES_MFMA": "0", "GL3_PF_PV_MFMA": "0"}, PREFILL),
         ({"GL3_PF_FUSED_ATTN": "0", "GL3_PF_SCORES_MFMA": "0", "GL3_PF_SCORES_PK": "0", "GL3_PF_PV_MFMA": "0"}, PREFILL),
         ({"GL3_PF_FUSED_MFMA": "0"}, PREFILL), ({"GL3_PF_FUSED_V1": "1"}, PREFILL),
         ({"GL3_NO_FUSED_BD_ATTN": "1"}, BATCHED), ({"GL3_NO_FUSED_QUANT": "1"}, BATCHED), ({"GL3_NO_FUSED_BD_ATTN": "1", "GL3_NO_FUSED_QUANT": "1"}, BATCHED)]


@pytest.mark.parametrize("env,sel", FORMS, ids=["-".join("%s=%s" % (k[4:], v) for k, v in e.items()) for e, _ in FORMS])
def test_the_all_model_under_each_form(env, sel):
    """The thirteen environments of test_gpu_gemm_forms.py.  The prefill forms run the > 64-token prefill (ragged-llama, tiny-devstral) and the
    attention regimes (prefill chunks of 256 under peaked attention: terms that are 0 or f32-subnormal, ties); the forms of the batched step
    run the > 64-token prefill and the step across position 128."""
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-k", sel, "-p", "no:cacheprovider"],
                         capture_output=True, text=True, timeout=300, env=dict(os.environ, **env), cwd=ROOT)
    tail = out.stdout[-1500:] + out.stderr[-500:]
    assert out.returncode == 0, tail
    assert "4 passed" in out.stdout and "failed" not in out.stdout and "skipped" not in out.stdout, tail


# ---- 9: one mixed step
@pytest.mark.parametrize("cfg", ["tiny-llama", "tiny-qwen3"])
def test_mixed_step_of_more_than_64_rows(pkg, orc, planmod, cfg):
    """Two decode rows (depths 5 and 9) and two prompt chunks (40 and 30 rows): 72 rows in one gl3_forward_batch."""
    plan_mod, _ = planmod
    m = em.make_edge_model(cfg, 8, 7, "all", ctx=64)
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=96, n_seqs=4)
    b = Mixed(orc, plan, [orc.COracle(m) for _ in range(4)], m, seed=19)
    b.prefill(0, 5)
    b.prefill(1, 9)
    c0, c1 = b.tokens(40), b.tokens(30)
    c0[7] = c0[8] = c1[0] = em.ZERO_TOKEN
    c1[3] = em.FLAT_TOKEN
    b.step([(0, [em.FLAT_TOKEN]), (2, c0), (1, [em.ZERO_TOKEN]), (3, c1)])
    assert b.pos == [6, 10, 40, 30]
    plan.freeTornadoExecutionPlan()


# ---- 10: MoE
MOE_EDITS = [("moe-router",), ("moe-router", "act-blocks", "w-scales"), "all"]


@pytest.mark.parametrize("edits", MOE_EDITS, ids=["router", "router+act+scales", "all"])
def test_moe_decode_prefill_and_batched_step(pkg, orc, planmod, edits):
    """Decode of 12 positions; batched prefill of 17 and of 96 tokens (x and the routing of every row, K / V of every position); one
    static-batched step whose 5 rows all make the same expert choice: one expert owns every row, six are empty; on the "all" model the
    second place is a seven-way tie at probability 0."""
    plan_mod, hip = planmod
    m = em.make_edge_model("tiny-qwen2moe", 8, 7, edits, ctx=160)
    plan = plan_mod.HipMasterPlan(m, flags=hip.FLAG_LAYER_TAPS)
    decode_and_compare([plan], orc.COracle(m), em.edge_tokens(pkg, m, 12))
    plan.freeTornadoExecutionPlan()
    for n in (17, 96):
        plan = plan_mod.HipMasterPlan(m, prefill_batch_size=96)
        o = orc.COracle(m)
        prefill_chunk_and_compare(plan, o, em.edge_tokens(pkg, m, n), 0)
        compare_kv(plan, o, n)
        plan.freeTornadoExecutionPlan()
    # w-scales without inner-act-blocks: one channel of x dominates and MOE_EXPERT's logit is negative for every token; another expert is full
    rows, choice = em.routed_tokens(m, 5, first=None if edits == MOE_EDITS[1] else em.MOE_EXPERT)
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=16, n_seqs=5)
    logits, ids = plan.forward_decode_batch(rows, list(range(5)), [0] * 5)
    sel = plan.buffer(10, 5 * m.cfg.n_experts_used).reshape(5, -1).astype(np.int32)
    assert sel.tolist() == [choice] * 5 and len(choice) == 2          # one expert owns every row, six of eight are empty
    for r, t in enumerate(rows):
        o = orc.COracle(m)
        ref = finite(o.forward(t, 0))
        assert np.array_equal(logits[r], ref) and int(ids[r]) == orc.argmax(ref), r
        for l in range(m.cfg.n_layers):
            k, v = plan.kv_seq(r, l, 0)
            ko, vo = o.kv(l, 0)
            assert np.array_equal(k, ko) and np.array_equal(v, vo), (r, l)
    plan.freeTornadoExecutionPlan()


# ---- 11: the native loader
@pytest.mark.parametrize("cfg,wtype", [("tiny-llama", 8), ("tiny-qwen3", 8), ("tiny-llama", 1), ("tiny-llama-tied", 2)])
def test_native_loader_keeps_the_edge_values(pkg, orc, planmod, tmp_path, cfg, wtype):
    """gl3_load_gguf on the "all" model written by write_gguf decodes bit-identically to the uploaded plan and to the oracle reading the same
    file: the repack into Q8T tiles keeps -128, zero / subnormal / negative / 2^15 scales."""
    plan_mod, hip = planmod
    m = em.make_edge_model(cfg, wtype, 7, "all")
    path = str(tmp_path / "edges.gguf")
    m.write_gguf(path)
    a = plan_mod.HipMasterPlan(m)
    b = plan_mod.HipMasterPlan.from_gguf(path)
    o = orc.COracle(pkg.synth.SynthModel.from_gguf(path), vector_bits=0 if wtype == 8 else 256)
    for pos, t in enumerate(em.edge_tokens(pkg, m, 10)):
        ref = finite(o.forward(t, pos))
        assert np.array_equal(a.forward_decode(t, pos), ref), ("uploaded", pos)
        assert np.array_equal(b.forward_decode(t, pos), ref), ("native", pos)
    a.freeTornadoExecutionPlan(); b.freeTornadoExecutionPlan()
