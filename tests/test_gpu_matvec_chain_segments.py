"""matvec_q8t_kernel<.., SEGS = true> sums a strip's block products in segments: the producers meet the chain wavefront at a workgroup
barrier after every batch of NPW x CH tile groups, and the chain wavefront adds that segment while the next one streams.  The launch
code picks it for strips of more than one segment and the one-pass chain (SEGS = false) otherwise, so K is placed on both sides of
that choice.  Order and rounding of the adds are those of one pass over the strip, so everything here is np.array_equal against the C
oracle: logits and x after every layer, under graph replay and with eager launches.

Segment length S in elements of K (128 per tile group), by launch class:
    gate/up (SwiGLU, two matrices)          NPW 4, CH 4:  16 groups = 2048      K = dim
    qkv, logits, wo / down with > 256 strips NPW 4, CH 8:  32 groups = 4096      K = dim (hidden for down)
    wo / down with <= 256 strips             NPW 8, CH 8:  64 groups = 8192      K = dim (hidden for down)
    routed experts (Qwen2-MoE, SEL)          NPW 4, always the one-pass chain (expert K is at most one segment in Qwen1.5-MoE-A2.7B)
K is placed around S: fewer groups than producer wavefronts, exactly one segment, one segment + 32 elements (a second segment of
one partial group; the group count is no multiple of NPW, so the wavefronts' tile counts differ), two segments - 96 elements, and
3.5 segments (the ratio of the 8B down projection).  dim = 32 x heads; hidden is free in multiples of 32.
"""
import functools

import numpy as np
import pytest

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu

STEPS = 4

# name -> (dim, hidden, heads, kv heads, vocab, layers)
CASES = {
    # K = 64 and 160: one and two tile groups, fewer than the 4 / 8 producer wavefronts; vocab 16400 = 1025 strips on 512 workgroups:
    # every workgroup runs two or three strips of the logits and the double buffer alternates
    "ng_below_npw_many_strips": (64, 160, 2, 1, 16400, 2),
    "ng_below_npw_swapped": (160, 64, 5, 1, 96, 2),
    # down, NPW 8 class (dim 64 = 4 strips), S = 8192
    "down_npw8_one_segment": (64, 8192, 2, 1, 96, 1),
    "down_npw8_one_segment_plus_32": (64, 8224, 2, 1, 96, 1),
    "down_npw8_two_segments_minus_96": (64, 16288, 2, 1, 96, 1),
    "down_npw8_three_and_a_half_segments": (64, 28672, 2, 1, 96, 2),
    # gate/up (SwiGLU), S = 2048; the same K runs qkv / logits / wo below, at or above their own segment length
    "swiglu_one_segment": (2048, 96, 64, 8, 80, 1),
    "swiglu_one_segment_plus_32": (2080, 96, 65, 5, 80, 1),
    "swiglu_two_segments_minus_96": (4000, 96, 125, 25, 80, 1),
    "swiglu_three_and_a_half_segments": (7168, 96, 224, 14, 80, 1),
    # qkv / logits, S = 4096: exactly one segment (wo: 256 strips, the NPW 8 class at half a segment)
    "qkv_one_segment": (4096, 96, 128, 8, 80, 1),
    # dim 4128 = 258 strips: wo and down take the NPW 4 residual class; qkv / logits / wo at one segment + 32, down at two segments - 96
    "npw4_residual_class": (4128, 8096, 129, 43, 80, 1),
}


@functools.lru_cache(maxsize=None)
def _reference(name):
    """The model and the oracle's logits / per-layer x of STEPS decode steps: computed once per case, shared by both launch modes."""
    from oracle import oracle_c
    oracle_c.build()
    pkg = ge.load_package()
    if name == "moe_tiny":
        cfg = pkg.synth.CONFIGS["tiny-qwen2moe"]            # K = 256 (gate/up) and 128 (down): two and one tile groups on the SEL launches
    else:
        dim, hidden, heads, kv, vocab, layers = CASES[name]
        assert dim == 32 * heads and heads % kv == 0 and hidden % 32 == 0
        cfg = pkg.synth.ModelConfig("chain-segments-" + name, pkg.synth.ARCH_LLAMA, dim, hidden, layers, heads, kv, 32, vocab, 16, 1e-5, 500000.0, False)
    m = pkg.synth.make_numpy(cfg, seed=41)
    o = oracle_c.COracle(m)
    toks = pkg.javarand.bench_tokens(m.cfg.vocab, STEPS)
    refs = []
    for pos, t in enumerate(toks):
        lg, lx = o.forward(t, pos, layer_x=True)
        refs.append((np.array(lg, copy=True), [np.array(x, copy=True) for x in lx]))
    for lg, lx in refs:
        lg.setflags(write=False)
        for x in lx:
            x.setflags(write=False)
    return m, toks, refs


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("name", list(CASES) + ["moe_tiny"])
def test_segmented_chain_is_bit_identical_to_the_oracle(name, graph):
    from importlib import import_module
    ge.load_package()
    plan_mod, hip = import_module(ge.PKG_NAME + ".plan"), import_module(ge.PKG_NAME + ".hip")
    m, toks, refs = _reference(name)
    plan = plan_mod.HipMasterPlan(m, flags=hip.FLAG_LAYER_TAPS | (0 if graph else hip.FLAG_NO_GRAPH))
    try:
        for pos, t in enumerate(toks):
            ref, lx = refs[pos]
            got = plan.tornadoVMForwardDecode(t, pos)
            for l in range(m.cfg.n_layers):
                assert np.array_equal(plan.layer_x(l), lx[l]), (name, pos, l)
            assert np.array_equal(got, ref), (name, pos)
    finally:
        plan.freeTornadoExecutionPlan()
