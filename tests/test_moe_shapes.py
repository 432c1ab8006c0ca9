"""What the Qwen2-MoE configuration grid (tests/moe_shapes.py) covers and the rule it states, checked without a GPU: the restated constants
against the kernel sources, the neighbours of gl3_create's limits (refused before any device call), the two oracles against each other at
every case, and the claims every case makes about its own routing."""
import ctypes as C
import os

import numpy as np
import pytest

import __graft_entry__ as ge
import moe_shapes as ms
from oracle import oracle_np

CSRC = os.path.join(ge.PKG_DIR, "csrc")
CASES = list(ms.GRID)


def test_the_grid_covers_every_branch():
    """Every class of the rule: where the gate row falls in the router's workgroups, the trips of the one-wavefront scan, the forms of the
    softmax sum, the top-k extremes, the shared slot counts and tails, the padded tile groups of the expert and shared K, and the batched
    grouping.  Dropping a row must fail."""
    assert ms.missing(CASES) == []
    for drop in CASES:
        assert ms.missing([n for n in CASES if n != drop]), "the grid covers the same without %s" % drop
    assert len(CASES) == 9
    assert {n: ms.GRID[n][:4] for n in CASES} == {
        "e1-k1": (1, 1, 128, 512), "e7-k7": (7, 7, 96, 320), "e8-k2-sh64": (8, 2, 128, 64), "e8-k2-sh128": (8, 2, 128, 128),
        "e63-k3": (63, 3, 32, 512), "e64-k8": (64, 8, 160, 1280), "e65-k4": (65, 4, 128, 512), "e64-k64": (64, 64, 32, 96),
        "e130-k6": (130, 6, 64, 160)}
    for name, (experts, topk, mh, hidden, _) in ms.GRID.items():
        assert 1 <= topk <= min(experts, ms.TOPK_MAX) and experts <= ms.EXPERTS_MAX and mh % 32 == 0 and hidden % 32 == 0 and mh and hidden, name


def test_the_rule():
    assert [ms.moe_router_wgs(e) for e in (1, 7, 8, 63, 64, 65, 130)] == [1, 1, 2, 8, 9, 9, 17]
    assert [ms.router_padding_rows(e) for e in (1, 7, 8, 63, 64, 65, 130)] == [6, 0, 7, 0, 7, 6, 5]
    assert [ms.gate_row_place(e) for e in (7, 8, 63, 64, 65)] == ["closes a full workgroup", "alone", "closes a full workgroup", "alone", "inside"]
    assert [ms.scan_trips(e) for e in (1, 64, 65, 128, 129, 130)] == [1, 1, 2, 2, 3, 3]
    assert ms.softmax_sum_form(1) == ("short", 0, 1) and ms.softmax_sum_form(7) == ("short", 1, 3) and ms.softmax_sum_form(8) == ("short", 2, 0)
    assert ms.softmax_sum_form(15) == ("short", 3, 3) and ms.softmax_sum_form(16) == ("pipelined", 0, 0)
    assert ms.softmax_sum_form(63) == ("pipelined", 1, 3) and ms.softmax_sum_form(64) == ("pipelined", 0, 0)
    assert ms.softmax_sum_form(65) == ("pipelined", 0, 1) and ms.softmax_sum_form(130) == ("pipelined", 0, 2)
    assert ms.shared_slot_rows(320, 96) == [96, 96, 96, 32] and ms.shared_slot_rows(64, 128) == [64] and ms.shared_slot_rows(128, 128) == [128]
    assert ms.shared_slot_rows(160, 64) == [64, 64, 32] and ms.shared_slot_rows(96, 32) == [32, 32, 32] and ms.shared_slots(1280, 160) == (8, 0)
    assert [ms.k_blocks(k) for k in (32, 64, 96, 128, 160, 320)] == [(1, 3), (2, 2), (3, 1), (4, 0), (5, 3), (10, 2)]
    assert ms.moe_group_max_entries(65, 64, 64) == 64 + 260 and ms.moe_group_max_entries(17, 6, 130) == 102 + 6
    assert [ms.experts_per_group_wave(e) for e in (8, 16, 17, 64, 65, 130)] == [1, 1, 2, 4, 5, 9]
    f = ms.facts("e64-k64")
    assert (f["slots"], f["terms"], f["rows_long"], f["expert_blocks"], f["shared_blocks"]) == (3, 65, 64 * 65, (1, 3), (3, 1))


def test_every_case_is_tiny_qwen2moe_with_four_fields_overridden(pkg):
    base = pkg.synth.CONFIGS["tiny-qwen2moe"].__dict__
    for name, (experts, topk, mh, hidden, _) in ms.GRID.items():
        c = ms.case_config(pkg.synth, name)
        assert (c.n_experts, c.n_experts_used, c.moe_hidden, c.hidden, c.ctx) == (experts, topk, mh, hidden, 96), name
        assert (c.dim, c.n_layers, c.n_heads, c.n_kv_heads, c.head_size, c.vocab) == (256, 2, 8, 2, 32, 512), name
        assert {k for k, v in c.__dict__.items() if v != base[k]} <= {"name", "ctx", "n_experts", "n_experts_used", "moe_hidden", "hidden"}, name


def test_the_constants_are_the_ones_in_the_kernel_sources():
    src = {f: open(os.path.join(CSRC, f)).read() for f in ("gl3_moe_kernels.h", "gl3_decode_kernels.h", "gl3_api.hip")}
    moe, dec, api = src["gl3_moe_kernels.h"], src["gl3_decode_kernels.h"], src["gl3_api.hip"]
    assert "constexpr int MOE_RR = %d;" % ms.MOE_RR in moe
    assert "return (n_experts + 1 + MOE_RR - 1) / MOE_RR;" in moe
    assert "return rr < E ? a.gate_inp + (size_t)rr * k : a.gate_inp_shexp;" in moe                 # padding rows alias the gate row
    assert "for (int i = t; i < E; i += %d)" % ms.WAVE in moe and "for (int j = t; j < E; j += %d) amx_take" % ms.WAVE in moe
    assert "if ((index & %d) == t) e[index] = -INFINITY;" % (ms.WAVE - 1) in moe
    assert "const float sum = seq_sum_lds<false>(e, E);" in moe
    assert "constexpr int MOE_GROUP_THREADS = %d;" % ms.MOE_GROUP_THREADS in moe and "nw = MOE_GROUP_THREADS / %d" % ms.WAVE in moe
    assert "return (n_experts < s ? n_experts : s) + s / 16;" in moe
    body = dec[dec.index("__device__ __forceinline__ float seq_sum_lds(const float* v, int n"):]
    body = body[:body.index("return s;")]
    assert "if (n >= %d) {" % ms.SUM_PIPELINE_MIN in body and "for (; i + 4 <= n; i += 4)" in body and "for (; i < n; ++i)" in body
    assert "if (left < a.rows) { a.rows = left; a.nstrips = (left + 15) / 16; }" in dec
    assert "(which == 0 ? (shared_rows + rows - 1) / rows : 0)" in api
    assert "d.n_experts > %d" % ms.EXPERTS_MAX in api and "d.n_experts_used > %d" % ms.TOPK_MAX in api
    assert "if (d.moe_hidden < 32 || d.moe_hidden % 32)" in api
    assert "int moe_sel[%d]; float moe_w[%d];" % (ms.TOPK_MAX, ms.TOPK_MAX) in open(os.path.join(ge.ROOT, "oracle", "gl3_oracle.c")).read()


@pytest.fixture(scope="module")
def hip():
    if not os.path.exists(os.path.join(ge.PKG_DIR, "libgpullama_hip.so")):
        ge.build()
    ge.load_package()
    from importlib import import_module
    return import_module(ge.PKG_NAME + ".hip")


def _create(hip, name, **over):
    """gl3_create on the description of the batched test's plan (max_batch 65, 3 sequences) -> (code, message); a plan that does get made (a
    machine with a GPU) is destroyed"""
    experts, topk, mh, hidden, _ = ms.GRID[name]
    d = hip.ModelDesc(C.sizeof(hip.ModelDesc), 5, ms.DIM, hidden, ms.LAYERS, ms.HEADS, ms.KV_HEADS, ms.HEAD_SIZE, ms.VOCAB, ms.CTX, 1e-6, 8, ms.LONG, 0, 0, 1,
                      0, 3, 1.0, 0.0, 1.0, 1.0, experts, topk, mh)
    for k, v in over.items():
        setattr(d, k, v)
    h = C.c_void_p()
    code = hip.lib().gl3_create(C.byref(d), C.byref(h))
    msg = (hip.lib().gl3_last_error(None) or b"").decode()
    if code == 0:
        hip.lib().gl3_destroy(h)
    return code, msg


def test_the_neighbours_of_the_limits_are_refused(hip):
    """Every case of the grid passes gl3_create's checks (without a device the call then ends in GL3_E_HIP at hipSetDevice); one step past a
    limit is GL3_E_ARG with a message that names the rule, before any device call."""
    for name in CASES:
        code, msg = _create(hip, name)
        assert code in (0, hip.E_HIP), (name, code, msg)
    assert _create(hip, "e64-k64", n_experts=4096)[0] in (0, hip.E_HIP)                       # the largest expert count
    counts = "1 <= n_experts_used <= min(n_experts, 64), n_experts <= 4096"
    for name, over in (("e65-k4", dict(n_experts_used=65)),             # top-k 65 with 65 experts: within n_experts, above the limit
                       ("e64-k64", dict(n_experts=63)),                 # top-k 64 of 63 experts
                       ("e1-k1", dict(n_experts_used=2)),               # top-k above the one expert
                       ("e1-k1", dict(n_experts=0)),
                       ("e130-k6", dict(n_experts=4097))):
        code, msg = _create(hip, name, **over)
        assert code == hip.E_ARG == -1 and counts in msg, (name, over, code, msg)
    for name, over in (("e63-k3", dict(moe_hidden=0)), ("e63-k3", dict(moe_hidden=48)), ("e63-k3", dict(moe_hidden=16))):
        code, msg = _create(hip, name, **over)
        assert code == hip.E_ARG and "moe_hidden must be a positive multiple of 32" in msg, (name, over, code, msg)


@pytest.mark.parametrize("name", CASES)
def test_both_oracles_agree(pkg, orc, name):
    """The C oracle is the GPU test's reference; here it meets the NumPy restatement at the same shapes: logits and the last layer's routing of
    4 tokens, bit for bit."""
    m = ms.case_model(pkg, name)
    co = orc.COracle(m)
    no = oracle_np.NpOracle(m.oracle_cfg(), m.oracle_tensors(), m.rope)
    topk = ms.GRID[name][1]
    for pos, t in enumerate(ms.decode_tokens(pkg)):
        a, b = co.forward(t, pos), no.forward(t, pos)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (name, "logits", pos)
        sel, w, sw = co.moe_routing()
        assert sel.tolist() == no.moe_sel and len(no.moe_sel) == topk, (name, "expert ids", pos)
        assert np.array_equal(w.view(np.uint32), np.array(no.moe_w, np.float32).view(np.uint32)), (name, "probabilities", pos)
        assert np.float32(sw).view(np.uint32) == np.float32(no.moe_shared_w).view(np.uint32), (name, "shared gate", pos)
    co.close()


def chunk_routing(pkg, orc, name):
    """The oracle's expert ids of the last layer for the 17- and the 65-token chunk of the batched GPU test"""
    m = ms.case_model(pkg, name)
    short, long_ = ms.chunk_tokens(pkg)
    out = []
    for toks in (short, long_[:ms.LONG]):
        o = orc.COracle(m)
        rows = []
        for b, t in enumerate(toks):
            o.prefill([t], b)
            rows.append(o.moe_routing()[0].tolist())
        o.close()
        out.append(rows)
    return out


@pytest.mark.parametrize("name", CASES)
def test_every_case_is_the_case_it_claims_to_be(pkg, orc, name):
    """The model seed of a case is picked so that the oracle alone selects expert 64 (e65-k4) or one >= 128 (e130-k6), leaves 28 experts empty
    at 17 tokens, fills 5 table entries per expert (e64-k64) or puts more than 16 assignments on one expert (e63-k3, e64-k8)."""
    short_sel, long_sel = chunk_routing(pkg, orc, name)
    assert ms.claims(name, short_sel, long_sel) == []


def test_the_claims_can_fail():
    """claims() on routings that do not meet them"""
    flat = lambda n, topk, experts: [[(r * topk + j) % experts for j in range(topk)] for r in range(n)]
    assert ms.claims("e63-k3", flat(17, 3, 63), flat(65, 3, 63)) == ["no expert holds more than 16 assignments at 65 tokens"]
    low = lambda n: [[0, 1, 2, 3]] * n
    assert ms.claims("e65-k4", low(17), low(65)) == ["no row selects expert 64"]
    low6 = lambda n: [[r % 100 + j for j in range(6)] for r in range(n)]
    assert "no row selects an expert >= 128" in ms.claims("e130-k6", low6(17), low6(65))
    assert ms.claims("e7-k7", [[0, 1, 2, 3, 4, 5, 5]] * 17, [list(range(7))] * 65)[0].startswith("a row's selection is not 7 distinct")
    assert ms.claims("e64-k64", [list(range(64))] * 17, [list(range(64))] * 65) == []
