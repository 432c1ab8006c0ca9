"""GL3_FLAG_KQUANT_NATIVE_MOE: Qwen2-MoE K-quant GGUFs whose stacked expert tensors stay native in HBM are bit-identical to the CPU oracle
on the NumPy-converted Q8_0 tensors: single-token decode (matvec_kq_kernel<.., SEL>), prompt chunks on both sides of 64 tokens, a
static-batched decode step and a mixed step (kq_gemm_grp_kernel), by the protocols of test_gpu_kquant_native(_batch).py.

  q4_k_m   everything native; 130 assignments over 8 experts at 65 tokens put more than 16 on one expert (a second entry in a workgroup)
  down-q8  a SwiGLU pair of two formats in the routed slots and another in the shared slot, which is smaller than one expert (tail); K = 128
           and 64 hold no super-block, so down_exps and the shared down stay Q8T beside native stacks and the down launch keeps its kernel
  e2-k2    top-k = E: 65 assignments per expert = five entries, a second workgroup with one ragged entry; two shared slots, one a tail
  segs     gate / up at K = 1792 and expert down at K = 3328: two chain segments each, the SEGS forms of the SEL kernel.  One layer: of a
           batched chunk only the last row's expert output reaches what is compared (its logits), so this case is about the decode
           forms; the grouped kernel is covered through the second layer's attention by the two-layer cases"""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest

import __graft_entry__ as ge
import moe_shapes as ms
from test_gpu_kquant_native import Q4_K, Q5_K, Q6_K, Q8_0, build, q4_k_m

pytestmark = pytest.mark.gpu


def down_q8(name):
    part = {"ffn_gate_exps": Q5_K, "ffn_up_exps": Q4_K, "ffn_down_exps": Q8_0, "ffn_down_shexp": Q8_0, "ffn_up_shexp": Q6_K}
    return next((t for k, t in part.items() if k in name), Q4_K)


#        id        dim   layers heads hs  experts top-k moe_hidden shared types             flags (1 = GL3_FLAG_NO_GRAPH)
CASES = [("q4_k_m",       256,  2, 8,  32,  8, 2, 256,  512, q4_k_m,           0),
         ("q4_k_m-eager", 256,  2, 8,  32,  8, 2, 256,  512, q4_k_m,           1),
         ("down-q8",      256,  2, 8,  32,  8, 2, 128,  64,  down_q8,          0),
         ("e2-k2",        256,  2, 8,  32,  2, 2, 512,  768, lambda n: Q6_K,   0),
         ("segs",         1792, 1, 14, 128, 2, 1, 3328, 256, lambda n: Q4_K,   0)]
MAXB, NSEQ = 80, 3


def model(case, tmp_path, tied=False):
    """(GGUF path of the K-quant file, the same model converted to Q8_0, config)"""
    name, dim, layers, heads, hs, experts, topk, mh, shared, types, _ = case
    synth = import_module(ge.PKG_NAME + ".synth")
    cfg = synth.ModelConfig(name, 5, dim, shared, layers, heads, 2, hs, ms.VOCAB, ms.CTX, 1e-6, 1000000.0, tied,
                            n_experts=experts, n_experts_used=topk, moe_hidden=mh)
    km, qm = build(synth, cfg, types, np.random.default_rng(79))
    path = str(tmp_path / "kq-moe.gguf")
    km.write_gguf(path)
    return path, qm, cfg


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_native_moe_plan_matches_the_oracle_on_converted_tensors(pkg, orc, tmp_path, case):
    hip, plan_mod = (import_module(ge.PKG_NAME + m) for m in (".hip", ".plan"))
    path, qm, cfg = model(case, tmp_path)
    flags = hip.FLAG_KQUANT_NATIVE_MOE | case[-1]
    # single-token entry points: four tokens through prefill, then decode steps
    toks = pkg.javarand.bench_tokens(cfg.vocab, 10)
    plan, o = plan_mod.HipMasterPlan.from_gguf(path, flags=flags), orc.COracle(qm)
    plan.prefill(toks[:4], 0)
    o.prefill(toks[:4], 0)
    for pos in range(4, 8):
        ref = o.forward(toks[pos], pos)
        assert np.isfinite(ref).all() and np.array_equal(plan.forward_decode(toks[pos], pos), ref), pos
    assert plan.forward_decode_sample(toks[8], 8, 0.0, 1.0, 0.0) == int(np.argmax(o.forward(toks[8], 8)))
    plan.freeTornadoExecutionPlan()
    # batched entry points: sequence 0 takes the 17-token chunk, sequence 1 the 65-token chunk, each against an oracle of its own
    plan = plan_mod.HipMasterPlan.from_gguf(path, prefill_batch_size=MAXB, flags=flags, n_seqs=NSEQ)
    chunks = [list(c) for c in ms.chunk_tokens(pkg)]
    after, chunks[1] = chunks[1][ms.LONG], chunks[1][:ms.LONG]
    oracles, busiest = [orc.COracle(qm) for _ in range(NSEQ)], 0
    for s, chunk in enumerate(chunks):
        n, sel = len(chunk), []
        for p, t in enumerate(chunk):
            ref = oracles[s].forward(t, p)
            sel += list(oracles[s].moe_routing()[0])
        busiest = max(sel.count(e) for e in set(sel))
        lg, ids = plan.forward_batch(chunk, [s] * n, range(n))
        assert np.isfinite(ref).all() and np.array_equal(lg[0], ref) and ids[0] == int(np.argmax(ref)), (s, n)
        for layer in range(cfg.n_layers):
            for p in (0, n - 1):
                assert all(np.array_equal(a, b) for a, b in zip(plan.kv_seq(s, layer, p), oracles[s].kv(layer, p))), (s, layer, p)
    if case[0].startswith("q4_k_m"):
        assert busiest > 16, busiest                  # the last layer's routing of the 65-token chunk: some expert owns two table entries
    depth = [ms.SHORT, ms.LONG, 0]                   # a static-batched decode step at mixed depths
    lg, ids = plan.forward_decode_batch([chunks[0][0], after, chunks[1][3]], range(NSEQ), depth)
    for s, (t, d) in enumerate(zip([chunks[0][0], after, chunks[1][3]], depth)):
        assert np.array_equal(lg[s], oracles[s].forward(t, d)), ("batched decode", s)
    rows = [(0, ms.SHORT + 1, after), (1, ms.LONG + 1, toks[0])] + [(2, 1 + p, t) for p, t in enumerate(chunks[0])]      # a mixed step
    lg, ids = plan.forward_batch([t for _, _, t in rows], [s for s, _, _ in rows], [p for _, p, _ in rows])
    refs = [oracles[s].forward(t, p) for s, p, t in rows]
    for got, ref in zip(lg, (refs[0], refs[1], refs[-1])):
        assert np.array_equal(got, ref)
    plan.freeTornadoExecutionPlan()


def test_weight_bytes_of_a_q6_k_moe_plan(pkg, tmp_path):
    """every matrix, the tied embedding and the expert stacks included, is Q6_K and every row count a multiple of 16: 28 of Q8T's 34 bytes"""
    hip, plan_mod = (import_module(ge.PKG_NAME + m) for m in (".hip", ".plan"))
    path, _, _ = model(CASES[3], tmp_path, tied=True)
    native, conv = plan_mod.HipMasterPlan.from_gguf(path, flags=hip.FLAG_KQUANT_NATIVE_MOE), plan_mod.HipMasterPlan.from_gguf(path)
    assert native.weight_bytes() * 34 <= conv.weight_bytes() * 28, (native.weight_bytes(), conv.weight_bytes())
    native.freeTornadoExecutionPlan()
    conv.freeTornadoExecutionPlan()
    # gl3_destroy gives the native stacks back: 16 more plans of 1.4 MB of expert segments each leave the device's free memory where it was
    rt, free, total = C.CDLL("libamdhip64.so"), C.c_size_t(), C.c_size_t()
    rt.hipMemGetInfo(C.byref(free), C.byref(total))
    before = free.value
    for _ in range(16):
        plan_mod.HipMasterPlan.from_gguf(path, flags=hip.FLAG_KQUANT_NATIVE_MOE).freeTornadoExecutionPlan()
    rt.hipMemGetInfo(C.byref(free), C.byref(total))
    assert before - free.value < 8 << 20, (before, free.value)


@pytest.mark.parametrize("what", [dict(tp_size=2), dict(flags=512 | 16)], ids=["tp_size", "f32_activation"])
def test_flag_is_refused_where_it_has_no_kernels(pkg, what):
    hip = import_module(ge.PKG_NAME + ".hip")
    d = hip.ModelDesc(struct_size=C.sizeof(hip.ModelDesc), arch=5, dim=256, hidden=512, n_layers=1, n_heads=8, n_kv_heads=2, head_size=32,
                      vocab=512, ctx=16, rms_eps=1e-5, weight_type=Q8_0, max_batch=8, tp_size=1, flags=hip.FLAG_KQUANT_NATIVE_MOE, n_seqs=1,
                      n_experts=4, n_experts_used=2, moe_hidden=64)
    for k, v in what.items():
        setattr(d, k, v)
    ctx = C.c_void_p()
    assert hip.lib().gl3_create(C.byref(d), C.byref(ctx)) == hip.E_UNSUPPORTED
    assert b"GL3_FLAG_KQUANT_NATIVE_MOE" in hip.lib().gl3_last_error(None)
