"""GL3_FLAG_KQUANT_NATIVE_BATCH: batched prefill, static-batched decode and mixed steps on native Q4_K / Q6_K storage are bit-identical
to the CPU oracle on the NumPy-converted Q8_0 tensors.

Every sequence of a test reads the same token stream, so one oracle pass over it per model (REF) holds the logits and K / V rows every
case compares with.  Step sizes sit on the boundaries of kq_gemm_kernel (token tiles of 16; 32 / 64 token slots; K = 256 is half a
stage of 4 tiles, 1536 three stages, 3328 six and a half) and past 64 tokens, where kq_expand_q8t_kernel feeds the Q8_0 GEMMs (65 and
130: a partial 128-token tile)."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest

import __graft_entry__ as ge
from test_gpu_kquant_native import Q6_K, Q8_0, build, mixed, phi3, q4_k_m

gpu = pytest.mark.gpu
NTOK, CTX, MAXB, NSEQ = 152, 160, 130, 34
#         id        arch dim   hidden layers heads kv hs   types
MODELS = {"q4_k_m": (0, 256,  768,  2,     8,    2, 32,  q4_k_m),
          "q6_k":   (0, 256,  768,  1,     8,    2, 32,  lambda n: Q6_K),
          "mixed":  (0, 256,  768,  1,     8,    2, 32,  mixed),
          "phi3":   (4, 256,  768,  2,     8,    8, 32,  phi3),
          "k1536":  (0, 1536, 3328, 1,     12,   2, 128, q4_k_m)}
REF, PLANS = {}, {}


def ref(name, pkg, orc, tmp_path_factory):
    """(GGUF path, tokens, oracle logits by position, oracle, config) of a model, made once"""
    if name not in REF:
        synth = import_module(ge.PKG_NAME + ".synth")
        arch, dim, hidden, layers, heads, kv, hs, types = MODELS[name]
        cfg = synth.ModelConfig(name, arch, dim, hidden, layers, heads, kv, hs, 528, CTX, 1e-5, 10000.0, False)
        km, qm = build(synth, cfg, types, np.random.default_rng(78))
        path = str(tmp_path_factory.mktemp(name) / "kq.gguf")
        km.write_gguf(path)
        toks = pkg.javarand.bench_tokens(cfg.vocab, NTOK)
        o = orc.COracle(qm)
        REF[name] = (path, toks, [o.forward(t, p) for p, t in enumerate(toks)], o, cfg)
    return REF[name]


def plan_of(name, path, flags=0):
    """one plan per (model, extra flags), shared by the cases of this module"""
    if (name, flags) not in PLANS:
        hip, plan_mod = (import_module(ge.PKG_NAME + m) for m in (".hip", ".plan"))
        PLANS[name, flags] = plan_mod.HipMasterPlan.from_gguf(path, prefill_batch_size=MAXB, flags=hip.FLAG_KQUANT_NATIVE_BATCH | flags, n_seqs=NSEQ)
    return PLANS[name, flags]


@gpu
@pytest.mark.parametrize("n", [1, 16, 17, 33, 64, 65, 130])
@pytest.mark.parametrize("name", MODELS)
def test_prompt_chunk(pkg, orc, tmp_path_factory, name, n):
    path, toks, logits, o, cfg = ref(name, pkg, orc, tmp_path_factory)
    plan = plan_of(name, path)
    plan.prefill(toks[:n], 0, batch=n)
    for layer in range(cfg.n_layers):
        for pos in (0, n - 1):
            assert all(np.array_equal(a, b) for a, b in zip(plan.kv(layer, pos), o.kv(layer, pos))), (layer, pos)
    lg, ids = plan.forward_batch(toks[:n], [1] * n, range(n))      # the same chunk as a mixed step's only run: its last row's logits
    assert np.array_equal(lg[0], logits[n - 1]) and ids[0] == int(np.argmax(logits[n - 1]))
    assert np.array_equal(plan.forward_decode(toks[n], n), logits[n])      # single-token decode (matvec_kq_kernel) over the chunk's K / V


@gpu
@pytest.mark.parametrize("case", [("q4_k_m", 2, 0), ("q4_k_m", 17, 0), ("q4_k_m", 33, 0), ("q4_k_m", 33, 1), ("mixed", 17, 0), ("phi3", 33, 0),
                                  ("k1536", 33, 0)], ids=lambda c: "%s-%d-%s" % (c[0], c[1], "eager" if c[2] else "graph"))
def test_static_batched_decode_at_mixed_depths(pkg, orc, tmp_path_factory, case):
    name, nseq, flags = case                                       # flags 1 = GL3_FLAG_NO_GRAPH
    path, toks, logits, o, cfg = ref(name, pkg, orc, tmp_path_factory)
    plan = plan_of(name, path, flags)
    plan.prefill_seq(0, toks[:NTOK - 1])
    plan.kv_seq_copy(0, list(range(1, nseq)), 0, NTOK - 1)
    for rep in range(2):                                           # a captured step replays: twice, the second at other depths
        depth = [(37 * i + 11 * rep) % (NTOK - 1) for i in range(nseq)]      # both sides of the short-context attention's limit
        lg, ids = plan.forward_decode_batch([toks[d] for d in depth], range(nseq), depth)
        for i, d in enumerate(depth):
            assert np.array_equal(lg[i], logits[d]) and ids[i] == int(np.argmax(logits[d])), (rep, i, d)


@gpu
@pytest.mark.parametrize("name", ["q4_k_m", "mixed", "k1536"])
def test_mixed_step_of_decode_rows_and_a_prompt_chunk(pkg, orc, tmp_path_factory, name):
    path, toks, logits, o, cfg = ref(name, pkg, orc, tmp_path_factory)
    plan = plan_of(name, path)
    plan.prefill_seq(0, toks[:100])
    plan.kv_seq_copy(0, [1, 2], 0, 100)
    rows = [(1, 40), (2, 99)] + [(3, p) for p in range(21)]        # two decode rows, then a chunk of 21 tokens of a fresh sequence
    lg, ids = plan.forward_batch([toks[p] for _, p in rows], [s for s, _ in rows], [p for _, p in rows])
    for got, pos in zip(lg, (40, 99, 20)):
        assert np.array_equal(got, logits[pos]), pos
    assert all(np.array_equal(a, b) for a, b in zip(plan.kv_seq(3, cfg.n_layers - 1, 20), o.kv(cfg.n_layers - 1, 20)))


@gpu
def test_score_of_more_than_64_rows_through_logits_slabs(pkg, orc, tmp_path_factory, monkeypatch):
    """70 logits rows: the 33 strips of the vocabulary matrix run as row slabs of 12, 12 and 9 strips of the smallest scratch"""
    monkeypatch.setenv("GL3_KQ_EXPAND_BYTES", "1")
    path, toks, logits, o, cfg = ref("q4_k_m", pkg, orc, tmp_path_factory)
    hip, plan_mod = (import_module(ge.PKG_NAME + m) for m in (".hip", ".plan"))
    plan = plan_mod.HipMasterPlan.from_gguf(path, prefill_batch_size=MAXB, flags=hip.FLAG_KQUANT_NATIVE_BATCH)      # its own: the scratch is sized at creation
    scores, ids = plan.forward_batch_score(toks[:70], [0] * 70, range(70), toks[1:71], want_logits=[1] * 70)
    assert np.array_equal(scores["logit"], np.array([logits[p][toks[p + 1]] for p in range(70)], np.float32))
    assert np.array_equal(scores["max"], np.array([logits[p].max() for p in range(70)], np.float32))
    assert ids.tolist() == [int(np.argmax(logits[p])) for p in range(70)]
    plan.freeTornadoExecutionPlan()


REFUSED = {"tp_size": dict(tp_size=2), "qwen2moe": dict(arch=5, n_experts=4, n_experts_used=2, moe_hidden=64), "f32_activation": dict(flags=256 | 16),
           "f16": dict(weight_type=1), "0x80 alone": dict(flags=128)}


@pytest.mark.parametrize("what", REFUSED)
def test_flag_is_refused_where_it_has_no_kernels(pkg, what):
    hip = import_module(ge.PKG_NAME + ".hip")
    d = hip.ModelDesc(struct_size=C.sizeof(hip.ModelDesc), arch=0, dim=256, hidden=512, n_layers=1, n_heads=8, n_kv_heads=2, head_size=32,
                      vocab=512, ctx=16, rms_eps=1e-5, weight_type=Q8_0, max_batch=8, tp_size=1, flags=hip.FLAG_KQUANT_NATIVE_BATCH, n_seqs=1)
    for k, v in REFUSED[what].items():
        setattr(d, k, v)
    ctx = C.c_void_p()
    assert hip.lib().gl3_create(C.byref(d), C.byref(ctx)) == hip.E_UNSUPPORTED
    assert b"GL3_FLAG_KQUANT_NATIVE_BATCH" in hip.lib().gl3_last_error(None)
