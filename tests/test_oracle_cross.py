"""The C oracle (timed CPU baseline) against the committed golden fixtures (made by the independent
NumPy restatement) — bit for bit — plus structural properties of the reference path."""
import os

import numpy as np
import pytest

from oracle import oracle_np

GOLD = os.path.join(os.path.dirname(__file__), "golden")
CASES = [("tiny_llama_q8_0", "tiny-llama", 8, 7, 0), ("tiny_llama_f16", "tiny-llama", 1, 7, 0),
         ("tiny_llama_tied_q4_0", "tiny-llama-tied", 2, 11, 0), ("tiny_qwen3_q8_0", "tiny-qwen3", 8, 5, 0),
         ("tiny_qwen2_q8_0", "tiny-qwen2", 8, 13, 0), ("tiny_granite_q8_0", "tiny-granite", 8, 19, 0), ("tiny_phi3_q8_0", "tiny-phi3", 8, 23, 0),
         ("tiny_devstral_q8_0", "tiny-devstral", 8, 29, 0), ("tiny_qwen2moe_q8_0", "tiny-qwen2moe", 8, 31, 0),
         # Vector-API dot order (256-bit species) for F16 / Q4_0 matrices: FP16FloatTensor.vectorDot / Q4_0FloatTensor.vectorDot
         ("tiny_llama_f16_v256", "tiny-llama", 1, 7, 256), ("tiny_llama_tied_q4_0_v256", "tiny-llama-tied", 2, 11, 256),
         # Q8_0 + 256 = -Dllama.quantizeActivation=false: Q8_0FloatTensor.vectorDot on the f32 activation (SURVEY 8 a4')
         ("tiny_llama_q8_0_f32act_v256", "tiny-llama", 8, 7, 256)]


@pytest.mark.parametrize("fx,cfg,wt,seed,vbits", CASES)
def test_c_oracle_matches_golden_bitwise(pkg, orc, fx, cfg, wt, seed, vbits):
    g = np.load(os.path.join(GOLD, fx + ".npz"))
    m = pkg.synth.make_numpy(pkg.synth.CONFIGS[cfg], wtype=wt, seed=seed)
    o = orc.COracle(m, vector_bits=vbits, f32_activation=(wt == 8 and vbits == 256))
    toks = g["tokens"]
    n_prompt = len(g["prompt"])
    assert toks[:n_prompt].tolist() == pkg.javarand.bench_tokens(m.cfg.vocab, n_prompt)
    for pos in range(g["logits"].shape[0]):
        lg, lx = o.forward(int(toks[pos]), pos, layer_x=True)
        assert np.array_equal(lg.view(np.uint32), g["logits"][pos].view(np.uint32)), pos
        if pos >= n_prompt - 1:
            assert orc.argmax(lg) == toks[pos + 1]            # greedy ids
    assert np.array_equal(lx, g["last_layer_x"])
    for l in range(m.cfg.n_layers):
        k, v = o.kv(l, g["logits"].shape[0] - 1)
        assert np.array_equal(k, g["k_last"][l]) and np.array_equal(v, g["v_last"][l])


def test_numpy_and_c_agree_on_fresh_seed(pkg, orc):
    # qwen2: q/k/v bias + NeoX RoPE; mha-llama: n_heads == n_kv_heads (kvMul = 1), head_size 128
    for cfg, wt in [("tiny-llama-tied", 8), ("tiny-qwen3", 1), ("tiny-qwen2", 8), ("tiny-qwen2", 2), ("mha-llama", 8), ("tiny-granite", 8), ("tiny-granite", 1), ("tiny-phi3", 8), ("tiny-phi3", 2),
                    ("tiny-devstral", 8), ("tiny-devstral", 1),        # devstral: q_dim 512 on dim 256, YaRN table
                    ("tiny-qwen2moe", 8), ("tiny-qwen2moe", 1)]:       # qwen2moe: F32 router, top-2 of 8 experts, gated shared expert
        m = pkg.synth.make_numpy(pkg.synth.CONFIGS[cfg], wtype=wt, seed=1234)
        co = orc.COracle(m)
        no = oracle_np.NpOracle(m.oracle_cfg(), m.oracle_tensors(), m.rope)
        for pos, t in enumerate(pkg.javarand.bench_tokens(m.cfg.vocab, 4, seed=9)):
            assert np.array_equal(co.forward(t, pos), no.forward(t, pos))


def test_numpy_and_c_agree_on_head_size_256_at_kvmul_16_and_qwen3_at_head_size_160(pkg, orc):
    """Two rows of the attention shape grid (tests/attn_shapes.py) that no config has: 16 query heads of 256 on one kv head (q_dim 4096 on dim 256),
    and Qwen3's per-head q / k RMSNorm + NeoX RoPE over 160 elements with 5 query heads per kv head.  tests/test_gpu_attn_shapes.py compares the
    kernels with the C oracle at these shapes; here the C oracle meets the NumPy restatement there first."""
    import attn_shapes as sh
    for name in ("llama-hs256-kv16", "qwen3-hs160-kv5"):
        m = sh.shape_model(pkg, name, ctx=64, seed=1234)
        assert (m.cfg.head_size, m.cfg.n_heads // m.cfg.n_kv_heads) in ((256, 16), (160, 5))
        co = orc.COracle(m)
        no = oracle_np.NpOracle(m.oracle_cfg(), m.oracle_tensors(), m.rope)
        for pos, t in enumerate(pkg.javarand.bench_tokens(m.cfg.vocab, 5, seed=9)):
            assert np.array_equal(co.forward(t, pos), no.forward(t, pos)), (name, pos)


def test_moe_routing_known_answers(orc):
    """InferenceCore.java:374-390 on hand-made router logits: the weights are the softmax over ALL experts (not renormalised over
    the chosen ones), selection is by strict > so the lowest index wins a tie, and the order is by descending probability."""
    import ctypes as C
    L = orc.lib()
    L.orc_moe_route.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.orc_moe_route.restype = None
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def route(logits, k):
        lg = np.array(logits, np.float32)
        sel, w = np.empty(k, np.int32), np.empty(k, np.float32)
        L.orc_moe_route(p(lg), lg.size, k, p(sel), p(w))
        return sel.tolist(), w
    # four equal logits: probabilities exactly 0.25 each, picked in index order
    sel, w = route([1.5, 1.5, 1.5, 1.5], 3)
    assert sel == [0, 1, 2] and w.tolist() == [0.25, 0.25, 0.25]
    # a tie between experts 1 and 3 for the top place: 1 first, then 3; weights sum to less than one
    sel, w = route([0.0, 2.0, -1.0, 2.0, 1.0], 2)
    assert sel == [1, 3] and w[0] == w[1] and 0.7 < float(w.sum()) < 0.8
    e = np.exp(np.array([0.0, 2.0, -1.0, 2.0, 1.0], np.float32).astype(np.float64) - 2.0).astype(np.float32)
    s = np.float32(0)
    for v in e:
        s = np.float32(s + v)                       # sequential f32 sum, FloatTensor.sum
    assert w[0] == np.float32(e[1] / s)
    # top-k = all experts: a full descending ordering with the softmax itself as weights
    sel, w = route([0.1, -0.3, 0.7, 0.2], 4)
    assert sel == [2, 3, 0, 1] and abs(float(w.sum()) - 1.0) < 1e-6 and all(w[i] > w[i + 1] for i in range(3))


def test_moe_block_structure(pkg, orc):
    """The MoE layer of the C oracle against an explicit NumPy composition of its parts for one token of tiny-qwen2moe: x_out =
    x + sum_j w_j * expert_j(xb) + sigmoid(g . xb) * shared(xb) accumulated in selection order (saxpy), each expert a SwiGLU FFN
    on the Q8_0 dot of the reference."""
    m = pkg.synth.make_numpy(pkg.synth.CONFIGS["tiny-qwen2moe"], seed=77)
    co = orc.COracle(m)
    no = oracle_np.NpOracle(m.oracle_cfg(), m.oracle_tensors(), m.rope)
    for pos, t in enumerate(pkg.javarand.bench_tokens(m.cfg.vocab, 5, seed=3)):
        a, b = co.forward(t, pos), no.forward(t, pos)
        assert np.array_equal(a, b)
        sel, w, sw = co.moe_routing()
        assert sel.tolist() == no.moe_sel and np.array_equal(w, np.array(no.moe_w, np.float32)) and sw == no.moe_shared_w
        assert len(set(sel.tolist())) == m.cfg.n_experts_used and w[0] >= w[1] and 0.0 < float(sw) < 1.0
        assert float(w.sum()) < 1.0                                               # not renormalised over the selected experts


def test_vector_api_dot_order_numpy_and_c_agree_and_stay_close_to_scalar(pkg, orc):
    """The 256-bit Vector-API dots (8 fused accumulator lanes, DAZ f16 conversion, lane-order reduce) in both restatements,
    on a seed that is not a fixture; the scalar and vector orders of the reference agree to ~1e-3 (F16: DAZ flushes the
    ~0.2 % subnormal weights) / ~1e-6 (Q4_0) relative, with identical greedy ids on these models."""
    for cfg, wt, tol in [("tiny-llama", 1, 2e-3), ("tiny-qwen3", 2, 1e-4), ("tiny-llama-tied", 2, 1e-4)]:
        m = pkg.synth.make_numpy(pkg.synth.CONFIGS[cfg], wtype=wt, seed=4321)
        cv, cs = orc.COracle(m, vector_bits=256), orc.COracle(m)
        nv = oracle_np.NpOracle(m.oracle_cfg(), m.oracle_tensors(), m.rope, vector_bits=256)
        for pos, t in enumerate(pkg.javarand.bench_tokens(m.cfg.vocab, 4, seed=9)):
            a, b, c = cv.forward(t, pos), nv.forward(t, pos), cs.forward(t, pos)
            assert np.array_equal(a, b), (cfg, pos)
            assert not np.array_equal(a, c)                                    # a different rounding order, visibly
            assert float(np.max(np.abs(a - c)) / np.max(np.abs(c))) < tol
            assert orc.argmax(a) == orc.argmax(c)


def test_q8_0_f32_activation_vector_dot_numpy_and_c_agree(pkg, orc):
    """SURVEY 8 a4': Q8_0FloatTensor.vectorDot (llama.quantizeActivation=false) in both restatements on a fresh seed, and against
    the default int8-activation path: different arithmetic (no activation rounding), so logits differ at the 1e-2 level while the
    greedy ids of these models agree."""
    for cfg in ("tiny-llama", "tiny-qwen3", "tiny-granite"):
        m = pkg.synth.make_numpy(pkg.synth.CONFIGS[cfg], wtype=8, seed=2468)
        cv, cq = orc.COracle(m, vector_bits=256, f32_activation=True), orc.COracle(m)
        nv = oracle_np.NpOracle(m.oracle_cfg(), m.oracle_tensors(), m.rope, vector_bits=256, f32_activation=True)
        for pos, t in enumerate(pkg.javarand.bench_tokens(m.cfg.vocab, 4, seed=9)):
            a, b, c = cv.forward(t, pos), nv.forward(t, pos), cq.forward(t, pos)
            assert np.array_equal(a, b), (cfg, pos)
            assert not np.array_equal(a, c)
            assert float(np.max(np.abs(a - c)) / np.max(np.abs(c))) < 5e-2


@pytest.mark.parametrize("bits", [128, 512])
def test_other_vector_species_numpy_and_c_agree(pkg, orc, bits):
    """FloatTensor.java:21 takes VectorShape.preferredShape(): 512 bits on an AVX-512 host (the GPU box's EPYC 9575F), 128 on SSE / NEON.
    FP16FloatTensor.vectorDot is species-generic (L = bits / 32 accumulator lanes); the Q8_0 / Q4_0 vector dots have a 128-bit branch
    (two fmas per block over 4-lane vectors, Q8_0FloatTensor.java:154-163, Q4_0FloatTensor.java:107-117) and THROW for 512
    (:165-167, :118-120).  Both restatements agree bit for bit in every mode the reference can run, differ from the 256-bit order, and
    raise where it throws."""
    cases = [("tiny-llama", 1, False), ("tiny-qwen3", 1, False), ("tiny-llama-tied", 2, False), ("tiny-llama", 8, True), ("tiny-phi3", 2, False)]
    for cfg, wt, f32act in cases:
        m = pkg.synth.make_numpy(pkg.synth.CONFIGS[cfg], wtype=wt, seed=1357)
        cv = orc.COracle(m, vector_bits=bits, f32_activation=f32act)
        c256 = orc.COracle(m, vector_bits=256, f32_activation=f32act)
        nv = oracle_np.NpOracle(m.oracle_cfg(), m.oracle_tensors(), m.rope, vector_bits=bits, f32_activation=f32act)
        toks = pkg.javarand.bench_tokens(m.cfg.vocab, 3, seed=9)
        if bits == 512 and wt != 1:
            with pytest.raises(orc.UnsupportedSpecies):
                cv.forward(toks[0], 0)
            with pytest.raises(oracle_np.UnsupportedSpecies):
                nv.forward(toks[0], 0)
            continue
        for pos, t in enumerate(toks):
            a, b, c = cv.forward(t, pos), nv.forward(t, pos), c256.forward(t, pos)
            assert np.array_equal(a, b), (cfg, bits, pos)
            assert not np.array_equal(a, c), (cfg, bits, pos)                  # another accumulator count = another rounding order
            assert float(np.max(np.abs(a - c)) / np.max(np.abs(c))) < 1e-3


def test_fma32_emulation_is_correctly_rounded():
    """oracle_np.fma32 (float64 product + round-to-odd sum) against exact rational arithmetic."""
    from fractions import Fraction
    rng = np.random.default_rng(5)
    a = rng.standard_normal(3000).astype(np.float32)
    b = rng.standard_normal(3000).astype(np.float32)
    c = (rng.standard_normal(3000) * rng.choice([1e-7, 1e-3, 1.0, 1e4], 3000)).astype(np.float32)
    got = oracle_np.fma32(a, b, c)
    for i in range(3000):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        f = np.float32(float(exact))
        cands = [np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))]
        best = min(cands, key=lambda z: (abs(Fraction(float(z)) - exact), int(np.float32(z).view(np.uint32)) & 1))
        assert best == got[i], i


def test_prefill_writes_the_same_kv_as_sequential_decode(pkg, orc):
    # InferenceCoreBatchPrefillDecode.batchForwardJavaPrefill :62-168 == forwardJava minus logits
    m = pkg.synth.make_numpy(pkg.synth.CONFIGS["tiny-llama"], seed=7)
    toks = pkg.javarand.bench_tokens(m.cfg.vocab, 9)
    a, b = orc.COracle(m), orc.COracle(m)
    for pos, t in enumerate(toks[:8]):
        a.forward(t, pos)
    b.prefill(toks[:5], 0)
    b.prefill(toks[5:8], 5)
    for l in range(m.cfg.n_layers):
        for pos in range(8):
            ka, va = a.kv(l, pos)
            kb, vb = b.kv(l, pos)
            assert np.array_equal(ka, kb) and np.array_equal(va, vb)
    assert np.array_equal(a.forward(toks[8], 8), b.forward(toks[8], 8))


def test_thread_count_independent(pkg, orc):
    import subprocess, sys, json
    code = ("import sys,json,numpy as np;sys.path.insert(0,%r);import __graft_entry__ as ge;p=ge.load_package();"
            "from oracle import oracle_c as oc;m=p.synth.make_numpy(p.synth.CONFIGS['tiny-llama'],seed=7);o=oc.COracle(m);"
            "o.forward(5,0);print(json.dumps(o.forward(9,1).view(np.uint32)[:64].tolist()))") % os.path.dirname(GOLD[:-6])
    outs = []
    for n in ("1", "3"):
        env = dict(os.environ, OMP_NUM_THREADS=n)
        outs.append(subprocess.check_output([sys.executable, "-c", code], env=env).decode().strip().splitlines()[-1])
    assert outs[0] == outs[1]
