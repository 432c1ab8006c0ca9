"""The paired form of the decode Q8_0 matvec (matvec_q8t_kernel<PRO_RMS, EPI_STORE, NPW 8>: one workgroup, one RMSNorm prologue, two adjacent
strips, two chain wavefronts) and the launch rule that picks it: one-layer Q8_0 models through forward_decode, graph replay and eager
launches, bit for bit against the C oracle for 3 decode steps (logits and x after the layer).

The rule (launch_q8t, gl3_api.hip) pairs a PRO_RMS / EPI_STORE launch (qkv, logits) of a single rank when a strip is at most one chain
segment (K <= 4096: 32 tile groups), the number of 16-row strips is even and every pair gets a workgroup of its own (strips / 2 <= 256).
A plan's qkv rows are head_size * (heads + 2 * kv heads) with head_size a multiple of 32, and its vocabulary is a multiple of 16
(gl3_create): qkv has at least 6 strips and always an even number, and no launch of this class has a ragged last strip.  So the two-strip
launch (one workgroup, both chain wavefronts) and the odd strip count the rule must reject are reached through the logits, and an even
strip count with rows that are no multiple of 16 cannot be built: the kernel's guards for it (rows past `rows`, the missing second strip
of a last pair) stay unreached, as the row guard of the four-producer form does.

    case               K      qkv strips       logits strips     what it is there for
    two_strips         1024   8  paired        2  paired         the smallest logits launch: 1 workgroup
    one_segment        4096   24 paired        6  paired         ng = 32 exactly: every producer issues its whole strip (8 tiles) up front
    padded_block       4064   24 paired        4  paired         127 blocks: the last tile group carries a zero-padded block
    below_producers    64     8  paired        2  paired         1 tile group: producers 1-3 and 5-7 have no tile and only meet the barriers
    odd_strips         1024   8  paired        3  four producers the rule rejects an odd strip count
    two_segments       4128   24 four prod.    6  four producers the rule rejects more than one segment: the segmented chain as before
"""
import functools

import numpy as np
import pytest

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu

STEPS = 3
HEAD_SIZE = 32

# name -> (dim, heads, kv heads, vocab); hidden 64, one layer
CASES = {
    "two_strips": (1024, 2, 1, 32),
    "one_segment": (4096, 8, 2, 96),
    "padded_block": (4064, 8, 2, 64),
    "below_producers": (64, 2, 1, 32),
    "odd_strips": (1024, 2, 1, 48),
    "two_segments": (4128, 8, 2, 96),
}


def paired(rows, k):
    """launch_q8t's rule for a PRO_RMS / EPI_STORE launch of one rank"""
    strips, groups = (rows + 15) // 16, (k // 32 + 3) // 4
    return groups <= 32 and strips % 2 == 0 and strips // 2 <= 256


def test_the_cases_sit_on_both_sides_of_the_rule():
    forms = {n: (paired(HEAD_SIZE * (h + 2 * kv), dim), paired(vocab, dim)) for n, (dim, h, kv, vocab) in CASES.items()}
    assert forms == {"two_strips": (True, True), "one_segment": (True, True), "padded_block": (True, True), "below_producers": (True, True),
                     "odd_strips": (True, False), "two_segments": (False, False)}
    assert CASES["two_strips"][3] // 16 == 2 and CASES["one_segment"][0] // 128 == 32 and CASES["padded_block"][0] // 32 == 127


@functools.lru_cache(maxsize=None)
def _reference(name):
    """The model, the tokens and the oracle's (logits, x after the layer) per step: computed once per case, read by both launch modes."""
    from oracle import oracle_c
    oracle_c.build()
    pkg = ge.load_package()
    dim, heads, kv, vocab = CASES[name]
    cfg = pkg.synth.ModelConfig("qkv-paired-" + name, pkg.synth.ARCH_LLAMA, dim, 64, 1, heads, kv, HEAD_SIZE, vocab, 16, 1e-5, 500000.0, False)
    m = pkg.synth.make_numpy(cfg, wtype=8, seed=47)
    o = oracle_c.COracle(m)
    toks = pkg.javarand.bench_tokens(vocab, STEPS)
    refs = []
    for pos, t in enumerate(toks):
        lg, lx = o.forward(t, pos, layer_x=True)
        lg, x0 = np.array(lg, copy=True), np.array(lx[0], copy=True)
        lg.setflags(write=False)
        x0.setflags(write=False)
        refs.append((lg, x0))
    o.close()
    return m, toks, refs


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("name", list(CASES))
def test_decode_is_bit_identical_to_the_oracle(name, graph):
    from importlib import import_module
    ge.load_package()
    plan_mod, hip = import_module(ge.PKG_NAME + ".plan"), import_module(ge.PKG_NAME + ".hip")
    m, toks, refs = _reference(name)
    plan = plan_mod.HipMasterPlan(m, flags=hip.FLAG_LAYER_TAPS | (0 if graph else hip.FLAG_NO_GRAPH))
    try:
        for pos, t in enumerate(toks):
            lg, x0 = refs[pos]
            got = plan.forward_decode(t, pos)
            assert np.array_equal(plan.layer_x(0), x0), (name, "x", pos)
            assert np.array_equal(got, lg), (name, "logits", pos)
    finally:
        plan.freeTornadoExecutionPlan()
