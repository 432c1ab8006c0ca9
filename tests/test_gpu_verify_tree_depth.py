"""The tiled form of draft-tree attention (score rows in HBM: the table scores kernels, pf_softmax_rows_tree_kernel, pf_pv_tree_kernel), bit for
bit against the CPU oracle run linearly along root paths, as test_gpu_verify_tree checks the other two forms.  GL3_PF_TREE_TILED_MIN (read in
gl3_create) takes the floors away so that 2-layer models reach the kernels at small depths; gl3_get_attn_rows says which form served the step."""
import numpy as np
import pytest

from test_gpu_verify_tree import SHAPES, TREES, draft_tree, model, planmod  # noqa: F401  (planmod: fixture)

pytestmark = pytest.mark.gpu
TILED, PAIR = 2, 3      # gl3_get_attn_rows: the trio's slot, the per-row pair's


def run_case(pkg, orc, planmod, shape, trees, ctx, form):
    """trees: [(tree name, policy, p0)], tree r on sequence r; form: the slot of attn_rows() that holds all rows of the step"""
    plan_mod, _ = planmod
    m, prompt = model(pkg, shape, ctx)
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=80, n_seqs=len(trees))
    toks, seqs, poss, pars, want, oracles = [], [], [], [], [], []
    for s, (tree, policy, p0) in enumerate(trees):
        o = orc.COracle(m)
        if p0:
            o.prefill(prompt[:p0], 0); plan.prefill_seq(s, prompt[:p0], 0)
        t, p, path, token = draft_tree(o, orc, m.cfg.vocab, p0, prompt[p0], TREES[tree], policy)
        row0 = len(toks)
        toks += t; poss += p; seqs += [s] * len(t)
        pars += [-1 if a < 0 else a + row0 for a in TREES[tree]]
        want.append((row0, len(t), p0, [row0 + i for i in path], token))
        oracles.append(o)
    res, path = plan.forward_batch_verify_tree(toks, seqs, poss, pars)
    assert list(plan.attn_rows()) == [len(toks) if i == form else 0 for i in range(4)], list(plan.attn_rows())
    for s, (row0, n, p0, wpath, token) in enumerate(want):
        acc = len(wpath) - 1
        assert (int(res["accepted"][s]), int(res["token"][s])) == (acc, token), (s, res, want)
        assert path[row0:row0 + n].tolist() == wpath + [-1] * (n - 1 - acc), (s, path, wpath)
        for l in range(m.cfg.n_layers):
            for j in range(acc + 1):
                k, v = plan.kv_seq(s, l, p0 + j)
                ko, vo = oracles[s].kv(l, p0 + j)
                assert np.array_equal(k, ko) and np.array_equal(v, vo), (s, l, j)
        got, _ = plan.forward_decode_batch([token], [s], [p0 + acc + 1])
        assert np.array_equal(got[0], oracles[s].forward(token, p0 + acc + 1)), s
    plan.freeTornadoExecutionPlan()


# hs128-kv4: scores on the matrix pipe, slots 575 .. 638 are past its one-launch limit (511).  hs64-kv8: two head groups; hs96-kv1: VALU
# scores, lanes past column 95 — neither has a one-launch kernel.  p0: no prefix, a prefix inside tile 0, p0 beside and on a tile edge, and the
# tree's slots 250 .. 313 across timestep 256.
CASES = [("hs128-kv4", "tree64", policy, 575, 704) for policy in ("first", "last")]
CASES += [(shape, tree, "last", p0, 352) for shape in ("hs64-kv8", "hs96-kv1") for tree in ("tree64", "bin15") for p0 in (0, 1, 63, 64, 250)]


@pytest.mark.parametrize("shape,tree,policy,p0,ctx", CASES)
def test_one_tree_on_the_tiled_form(pkg, orc, planmod, monkeypatch, shape, tree, policy, p0, ctx):
    monkeypatch.setenv("GL3_PF_TREE_TILED_MIN", "0,1")
    run_case(pkg, orc, planmod, shape, [(tree, policy, p0)], ctx, TILED)


def test_two_trees_of_two_sequences_on_the_tiled_form(pkg, orc, planmod, monkeypatch):
    monkeypatch.setenv("GL3_PF_TREE_TILED_MIN", "0,1")
    run_case(pkg, orc, planmod, "hs64-kv8", [("bin15", "last", 250), ("star7", "first", 3)], 352, TILED)


def test_a_slot_floor_past_the_context_keeps_the_pair(pkg, orc, planmod, monkeypatch):
    monkeypatch.setenv("GL3_PF_TREE_TILED_MIN", "1000000,1")
    run_case(pkg, orc, planmod, "hs64-kv8", [("tree64", "last", 250)], 352, PAIR)


def test_the_default_floors(pkg, orc, planmod, monkeypatch):
    """64 rows ending at slot 1093 are past both default floors (last slot >= 1024, rows >= 32) and past the one-launch limit of the shape."""
    monkeypatch.delenv("GL3_PF_TREE_TILED_MIN", raising=False)
    run_case(pkg, orc, planmod, "hs128-kv4", [("tree64", "first", 1030)], 1100, TILED)
