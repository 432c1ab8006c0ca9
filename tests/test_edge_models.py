"""The edge models of tests/edge_models.py reach the conditions they are built for — shown by the reference oracles alone, on the CPU.

survey() runs the NumPy oracle with its taps over the token list the GPU tests use (edge_models.edge_tokens) and classifies every
matmul input block as the reference's activation quantiser (orc_quantize_act of the C oracle) sees it.  The figures asserted here are
properties of the test models, not of the code under test."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import edge_models as em
from oracle import oracle_np

N_TOKENS = 12
CONSUMERS = {"qkv": ("attn_q.weight",), "wo": ("attn_output.weight",), "gate/up": ("ffn_gate.weight", "ffn_gate_shexp.weight", "ffn_gate_exps.weight"),
             "down": ("ffn_down.weight", "ffn_down_shexp.weight", "ffn_down_exps.weight")}


def quantize_act(orc, x):
    L = orc.lib()
    x = np.ascontiguousarray(x, np.float32)
    q, s = np.empty(x.size, np.int8), np.empty(x.size // 32, np.float32)
    L.orc_quantize_act(x.ctypes.data_as(C.c_void_p), x.size, q.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p))
    return q.reshape(-1, 32), s


def is_f16_subnormal(s):
    return (s > 0) & (s < np.float32(2.0 ** -14))


@functools.lru_cache(maxsize=None)
def survey(cfg_name, **over):
    from oracle import oracle_c as orc
    orc.build()
    pkg = em.ge.load_package()
    m = em.make_edge_model(cfg_name, 8, 7, "all", **dict(over))
    o = oracle_np.NpOracle(m.oracle_cfg(), m.oracle_tensors(), m.rope)
    o.mm_taps, o.attn_taps = [], []
    toks = em.edge_tokens(pkg, m, N_TOKENS)
    finite, layer_max = True, 0.0
    for pos, t in enumerate(toks):
        lx = []
        lg = o.forward(t, pos, layer_x=lx)
        finite &= bool(np.all(np.isfinite(lg)) and np.all(np.isfinite(np.stack(lx))))
        layer_max = max(layer_max, float(np.max(np.abs(np.stack(lx)))))
    finite &= bool(np.all(np.isfinite(o.kc)) and np.all(np.isfinite(o.vc)))
    classes = {}                    # (layer, consumer) -> set of block classes seen
    max_isum, min_prod = 0, np.inf
    for name, row0, x in o.mm_taps:
        if not name.startswith("blk."):
            continue
        l, rest = int(name.split(".")[1]), name.split(".", 2)[2]
        cons = [k for k, v in CONSUMERS.items() if rest in v]
        if not cons:
            continue
        q, s = quantize_act(orc, x)
        aq, s_np = oracle_np.quantize_act(x)
        assert np.array_equal(aq, q.astype(np.int32)) and np.array_equal(s_np, s)      # both restatements of the quantiser agree on these
        nz = np.any(q != 0, axis=1)
        seen = classes.setdefault((l, cons[0]), set())
        if np.any((s == 0) & ~nz):
            seen.add("zero")
        if np.any((s == 0) & nz):
            seen.add("scale0-quants")
        if np.any(is_f16_subnormal(s)):
            seen.add("subnormal")
        if np.any(s >= 1):
            seen.add("big")
        raw, ty = o.t[name]
        d0 = {"qkv": m.cfg.q_dim, "wo": m.cfg.dim, "gate/up": m.cfg.moe_hidden if "exps" in name else m.cfg.hidden, "down": m.cfg.dim}[cons[0]]
        nb = x.size // 32
        blk = raw.view(np.uint8).reshape(-1)[row0 * nb * 34:(row0 + d0) * nb * 34].reshape(d0, nb, 34)
        ws = blk[:, :, :2].copy().view(np.float16).astype(np.float32).reshape(d0, nb)
        isum = np.einsum("rbi,bi->rb", blk[:, :, 2:].view(np.int8).astype(np.int64), q.astype(np.int64))
        max_isum = max(max_isum, int(np.max(np.abs(isum))))
        prod = np.abs(ws * s[None, :])
        if np.any(prod > 0):
            min_prod = min(min_prod, float(np.min(prod[prod > 0])))
    terms = dict(zero=0, subnormal=0, tie=0, flat=0)
    for l, h, pos, score in o.attn_taps:
        mx = np.max(score)
        e = np.exp((score - mx).astype(np.float64)).astype(np.float32)
        terms["zero"] += int(np.any(e == 0))
        terms["subnormal"] += int(np.any((e > 0) & (e < np.float32(2.0 ** -126))))
        terms["tie"] += int(np.sum(score == mx) >= 2)
        terms["flat"] += int(pos >= 3 and float(np.max(oracle_np.softmax(score))) < 0.5 and np.sum(score == mx) == 1)
    return dict(model=m, toks=toks, finite=finite, layer_max=layer_max, classes=classes, max_isum=max_isum, min_prod=min_prod, terms=terms)


# tiny-llama and tiny-qwen2moe have two 32-row groups of V (one zero, one ordinary): their f16-subnormal block into wo comes from
# edge_models.sink_head; the four-group variant of tiny-llama (n_kv_heads = 4) and tiny-qwen3 also get it from the shrunk V groups
MODELS = [("tiny-llama", ()), ("tiny-llama", (("n_kv_heads", 4),)), ("tiny-qwen3", ()), ("tiny-qwen2moe", ())]


@pytest.mark.parametrize("cfg,over", MODELS, ids=["tiny-llama", "tiny-llama-kv4", "tiny-qwen3", "tiny-qwen2moe"])
def test_every_consumer_sees_every_block_class(cfg, over):
    s = survey(cfg, **dict(over))
    m = s["model"]
    for l in range(m.cfg.n_layers):
        for cons in CONSUMERS:
            want = {"zero", "subnormal", "big"}
            if cons in ("qkv", "gate/up"):
                want.add("scale0-quants")                   # act-blocks only: the norm-fed consumers
            assert want <= s["classes"][(l, cons)], (cfg, l, cons, s["classes"][(l, cons)])


@pytest.mark.parametrize("cfg,over", MODELS, ids=["tiny-llama", "tiny-llama-kv4", "tiny-qwen3", "tiny-qwen2moe"])
def test_block_dot_bound_small_products_and_finiteness(cfg, over):
    s = survey(cfg, **dict(over))
    assert s["max_isum"] >= 400000, s["max_isum"]
    assert s["min_prod"] < 2.0 ** -40, s["min_prod"]
    assert s["finite"]
    assert s["layer_max"] < 1e17                              # squares of the residual stream stay finite in f32 as well


@pytest.mark.parametrize("cfg,over", [("tiny-llama", ()), ("tiny-llama", (("n_kv_heads", 4),)), ("tiny-qwen3", ())], ids=["tiny-llama", "tiny-llama-kv4", "tiny-qwen3"])
def test_softmax_terms(cfg, over):
    t = survey(cfg, **dict(over))["terms"]
    assert t["zero"] > 0 and t["subnormal"] > 0 and t["tie"] > 0 and t["flat"] > 0, t


def test_moe_router_tie_full_expert_and_empty_experts():
    """The step the GPU test runs: 5 rows that all route to (MOE_EXPERT, 0) in both layers — MOE_EXPERT's probability is 1, the other seven
    are exactly 0 and tie for the second place (lowest index wins): one expert has every row, six of eight have none.  Other tokens of the
    stream take the identical rows 1 and 2 together, with equal non-zero weights (the tie inside the top-k)."""
    m = em.make_edge_model("tiny-qwen2moe", 8, 7, "all")
    toks, choice = em.routed_tokens(m, 5)
    assert len(set(toks)) == 5 and choice == [em.MOE_EXPERT, 0]
    for edits in ("moe-router", ("moe-router", "act-blocks", "w-scales")):          # the other models of the GPU case: two experts in use, six empty
        first = em.MOE_EXPERT if edits == "moe-router" else None
        assert len(em.routed_tokens(em.make_edge_model("tiny-qwen2moe", 8, 7, edits, ctx=160), 5, first=first)[1]) == 2
    o = oracle_np.NpOracle(m.oracle_cfg(), m.oracle_tensors(), m.rope)
    for t in toks:
        o.moe_taps = []
        o.forward(t, 0, want_logits=False)
        assert [(sel, [float(w) for w in wts]) for _, sel, wts in o.moe_taps] == [([em.MOE_EXPERT, 0], [1.0, 0.0])] * m.cfg.n_layers
    pair = 0
    for t in range(64):
        o.moe_taps = []
        o.forward(t, 0, want_logits=False)
        for _, sel, wts in o.moe_taps:
            if sel == [1, 2]:
                assert wts[0] == wts[1] > 0, (t, wts)
                pair += 1
    assert pair > 0


def test_both_oracles_agree_on_the_all_model(orc):
    pkg = em.ge.load_package()
    for cfg, wt, kw in [("tiny-llama", 8, {}), ("tiny-qwen3", 8, {}), ("tiny-qwen2moe", 8, {}), ("tiny-phi3", 8, {}),
                        ("tiny-llama", 1, dict(vector_bits=256)), ("tiny-llama-tied", 2, dict(vector_bits=256)), ("tiny-llama", 1, {})]:
        m = em.make_edge_model(cfg, wt, 7, "all")
        toks = em.edge_tokens(pkg, m, 10)
        co, cp = orc.COracle(m, **kw), orc.COracle(m, **kw)
        no = oracle_np.NpOracle(m.oracle_cfg(), m.oracle_tensors(), m.rope, **kw)
        cp.prefill(toks[:8], 0)
        for pos, t in enumerate(toks):
            a, b = co.forward(t, pos), no.forward(t, pos)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (cfg, wt, pos)
            assert np.all(np.isfinite(a))
            if pos >= 8:
                assert np.array_equal(cp.forward(t, pos).view(np.uint32), a.view(np.uint32)), (cfg, wt, pos)
        for l in range(m.cfg.n_layers):
            for pos in range(8):
                ka, va = co.kv(l, pos)
                kb, vb = cp.kv(l, pos)
                assert np.array_equal(ka, kb) and np.array_equal(va, vb)
                assert np.array_equal(ka, no.kc[l, pos]) and np.array_equal(va, no.vc[l, pos])


def test_edits_are_deterministic_and_named():
    a = em.make_edge_model("tiny-llama", 8, 7, "all")
    b = em.make_edge_model("tiny-llama", 8, 7, em.EDITS)
    plain = em.ge.load_package().synth.make_numpy(a.cfg, wtype=8, seed=7)
    assert all(np.array_equal(a.tensors[k][0], b.tensors[k][0]) for k in a.tensors)
    for e in em.edits_for(8, 0, "all"):
        one = em.make_edge_model("tiny-llama", 8, 7, e)
        assert any(not np.array_equal(one.tensors[k][0], plain.tensors[k][0]) for k in one.tensors), e
    with pytest.raises(AssertionError):
        em.make_edge_model("tiny-llama", 8, 7, "no-such-edit")


def test_c_oracle_matches_the_edge_fixture_bitwise(orc):
    """tests/golden/tiny_llama_q8_0_edges.npz (made by the NumPy oracle, tests/golden/make_golden.py) against the C oracle."""
    pkg = em.ge.load_package()
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "tiny_llama_q8_0_edges.npz"))
    m = em.make_edge_model("tiny-llama", 8, 7, "all")
    o = orc.COracle(m)
    toks, n_prompt, steps = g["tokens"], len(g["prompt"]), g["logits"].shape[0]
    assert toks[:n_prompt].tolist() == em.edge_tokens(pkg, m, n_prompt)
    for pos in range(steps):
        lg, lx = o.forward(int(toks[pos]), pos, layer_x=True)
        assert np.array_equal(lg.view(np.uint32), g["logits"][pos].view(np.uint32)), pos
        if pos >= n_prompt - 1:
            assert orc.argmax(lg) == toks[pos + 1]
    assert np.array_equal(lx, g["last_layer_x"])
    for l in range(m.cfg.n_layers):
        k, v = o.kv(l, steps - 1)
        assert np.array_equal(k, g["k_last"][l]) and np.array_equal(v, g["v_last"][l])


def test_the_models_of_the_gpu_cases_stay_finite(orc):
    """Every (config, type, mode, edit) the GPU file runs, through the C oracle over the edge tokens: logits and x finite.  A large block
    scale in front of a quantised activation can push THAT activation's f16 scale to infinity; such a model tests nothing."""
    pkg = em.ge.load_package()
    cases = [("tiny-llama", 8, e, {}, {}) for e in em.edits_for(8, 0, "all")]
    cases += [(c, 8, e, {}, {}) for c, e in (("tiny-qwen3", "act-blocks"), ("tiny-qwen2", "all"), ("tiny-granite", "all"), ("tiny-phi3", "all"),
                                             ("tiny-phi3", "inner-act-blocks"))]
    cases += [(c, 8, e, dict(ctx=200), {}) for c, e in (("ragged-llama", "all"), ("tiny-devstral", "all"), ("ragged-llama", "act-blocks"),
                                                        ("ragged-llama", "w-scales"), ("ragged-llama", "inner-act-blocks"))]
    cases += [("tiny-qwen2moe", 8, e, {}, {}) for e in (("moe-router",), ("moe-router", "act-blocks", "w-scales"))]
    for c in ("tiny-llama", "tiny-llama-tied"):
        cases += [(c, 1, "all", dict(ctx=64), dict(vector_bits=v)) for v in (0, 256, 512)] + [(c, 2, "all", dict(ctx=64), dict(vector_bits=v)) for v in (0, 256)]
        cases += [(c, 8, "all", dict(ctx=64), dict(vector_bits=256, f32_activation=True))]
    for cfg, wt, edits, over, okw in cases:
        m = em.make_edge_model(cfg, wt, 7, edits, **over)
        o = orc.COracle(m, **okw)
        for pos, t in enumerate(em.edge_tokens(pkg, m, 24)):
            assert np.all(np.isfinite(o.forward(t, pos))) and np.all(np.isfinite(o.x())), (cfg, wt, edits, okw, pos)
