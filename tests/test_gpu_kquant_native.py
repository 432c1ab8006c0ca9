"""GL3_FLAG_KQUANT_NATIVE: K-quant GGUFs whose Q4_K / Q6_K tensors stay native in HBM decode bit-identically to the CPU oracle on the
NumPy-converted Q8_0 tensors — the check tests/test_gpu_kquant.py makes of the load-time conversion.

Shapes sit on each side of the boundaries of matvec_kq_kernel's plan (12 producers; one chain segment = 24 tile groups, 12 for
gate/up): K = 256 (one super-block), 768 (6 groups: fewer than the producers), 1536 | 1792 (gate/up: one | two segments) and
3072 | 3328 (qkv, logits, wo, down: one | two segments; 26 and 14 groups are no multiple of 12).  Of the kernel's RMS prologue
these reach the single-wavefront sum of squares (K = 256, 768) and the exact parallel one with the row in registers (1536 to 3328);
dim 5376, the first multiple of 256 above 5120, reaches the third form: the row re-read in a loop and the single-wavefront sum again.
gl3_create accepts vocabularies that are multiples of 16 only, so 528 (33 strips) stands in for a ragged vocabulary."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest

import __graft_entry__ as ge
import kquant_np as kq

pytestmark = pytest.mark.gpu
Q8_0, Q4_K, Q5_K, Q6_K = 8, 12, 13, 14


def q4_k_m(name):
    return Q6_K if ("attn_v" in name or "ffn_down" in name or name == "output.weight") else Q4_K


def mixed(name):        # a converted Q5_K segment between native ones in wqkv, and a SwiGLU pair of Q4_K and Q8T
    return Q5_K if "attn_k" in name else Q8_0 if "ffn_up" in name else q4_k_m(name)


def phi3(name):         # fused attn_qkv / ffn_up (= gate | up) tensors
    return Q6_K if ("ffn_" in name or name == "output.weight") else Q4_K


#        id            arch dim   hidden layers heads kv hs  tied   types                 flags (1 = GL3_FLAG_NO_GRAPH)
CASES = [("q4_k_m",      0, 256,  768,  2,     8,    2, 32,  False, q4_k_m,               0),
         ("q4_k_m-eager", 0, 256, 768,  2,     8,    2, 32,  False, q4_k_m,               1),
         ("q4_k-tied",   0, 1536, 3072, 1,     12,   2, 128, True,  lambda n: Q4_K,       0),
         ("q6_k",        0, 1792, 3328, 1,     14,   2, 128, False, lambda n: Q6_K,       0),
         ("mixed",       0, 3328, 512,  1,     26,   2, 128, False, mixed,                0),
         ("q4_k_m-5376", 0, 5376, 256,  1,     42,   6, 128, False, q4_k_m,               0),
         ("phi3",        4, 256,  512,  2,     8,    8, 32,  False, phi3,                 0)]


def build(synth, cfg, types, rng):
    """(K-quant model as the file holds it, the same model converted to Q8_0 by kquant_np)."""
    kt, q8 = {}, {}
    for name, rows, cols, ty, kind in synth.tensor_specs(cfg, Q8_0):
        t = types(name) if kind == "mat" else ty
        if t in (Q8_0, synth.GGML_F32):
            w = rng.standard_normal((rows, cols), dtype=np.float32) * np.float32(0.02) + np.float32(kind == "norm")
            kt[name] = q8[name] = (synth.encode(w, t), t, rows, cols)
            continue
        raw = kq.random_blocks(t, rows * cols, rng, scale=4e-3 if t == Q6_K else 1.5e-3)
        kt[name] = (raw, t, rows, cols)
        q8[name] = (kq.to_q8_0(kq.DEQUANT[t](raw, rows * cols)), Q8_0, rows, cols)
    return synth.SynthModel(cfg, Q8_0, kt), synth.SynthModel(cfg, Q8_0, q8)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_native_kquant_plan_matches_the_oracle_on_converted_tensors(pkg, orc, tmp_path, case):
    name, arch, dim, hidden, layers, heads, kv, hs, tied, types, flags = case
    hip, plan_mod, synth = (import_module(ge.PKG_NAME + m) for m in (".hip", ".plan", ".synth"))
    cfg = synth.ModelConfig(name, arch, dim, hidden, layers, heads, kv, hs, 528, 16, 1e-5, 10000.0, tied)
    km, qm = build(synth, cfg, types, np.random.default_rng(77))
    path = str(tmp_path / "kq.gguf")
    km.write_gguf(path)
    plan = plan_mod.HipMasterPlan.from_gguf(path, flags=hip.FLAG_KQUANT_NATIVE | flags)
    o = orc.COracle(qm)
    toks = pkg.javarand.bench_tokens(cfg.vocab, 12)
    plan.prefill(toks[:4], 0)
    o.prefill(toks[:4], 0)
    for pos in range(4, 10):
        assert np.array_equal(plan.forward_decode(toks[pos], pos), o.forward(toks[pos], pos)), pos
    assert plan.forward_decode_sample(toks[10], 10, 0.0, 1.0, 0.0) == int(np.argmax(o.forward(toks[10], 10)))
    if name in ("q4_k-tied", "q6_k"):      # every row count is a multiple of 16: 19 of Q8T's 34 bytes per block, and 28 of 34
        conv = plan_mod.HipMasterPlan.from_gguf(path)
        num = 20 if name == "q4_k-tied" else 28
        assert plan.weight_bytes() * 34 <= conv.weight_bytes() * num, (plan.weight_bytes(), conv.weight_bytes())
        conv.freeTornadoExecutionPlan()
    if name == "q4_k_m":                    # the other single-token entry points on the same plan
        assert plan.forward_decode_chain(toks[11], 11, 3)[0] == int(np.argmax(o.forward(toks[11], 11)))
        assert plan.profile_decode(toks[4], 4)["matvec_qkv"]["launches"] == layers
    plan.freeTornadoExecutionPlan()


REFUSED = {"tp_size": dict(tp_size=2), "max_batch": dict(max_batch=8), "n_seqs": dict(n_seqs=2), "f32_activation": dict(flags=128 | 16),
           "qwen2moe": dict(arch=5, n_experts=4, n_experts_used=2, moe_hidden=64), "f16": dict(weight_type=1)}


@pytest.mark.parametrize("what", REFUSED)
def test_native_kquant_flag_is_refused_where_it_has_no_kernels(what):
    hip = import_module(ge.PKG_NAME + ".hip")
    d = hip.ModelDesc(struct_size=C.sizeof(hip.ModelDesc), arch=0, dim=256, hidden=512, n_layers=1, n_heads=8, n_kv_heads=2, head_size=32,
                      vocab=512, ctx=16, rms_eps=1e-5, weight_type=Q8_0, max_batch=1, tp_size=1, flags=hip.FLAG_KQUANT_NATIVE, n_seqs=1)
    for k, v in REFUSED[what].items():
        setattr(d, k, v)
    ctx = C.c_void_p()
    assert hip.lib().gl3_create(C.byref(d), C.byref(ctx)) == hip.E_UNSUPPORTED
    assert b"GL3_FLAG_KQUANT_NATIVE" in hip.lib().gl3_last_error(None)
