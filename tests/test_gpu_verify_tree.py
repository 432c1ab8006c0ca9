"""gl3_forward_batch_verify_tree on the GPU, bit for bit against the CPU oracle run linearly along root paths: 2-layer synthetic Q8_0 models,
drafts built from the oracle's own greedy continuation.  Per case: results and path, the K / V rows of the accepted path at positions
p0 .. p0 + accepted in every layer, and the logits of the decode step that follows at p0 + accepted + 1."""
import ctypes

import numpy as np
import pytest

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu
CTX = 160
# name -> (head size, heads, kv heads); the first two run pf_attn_tree_kernel (gl3_get_attn_rows()[1]), the others the masked per-row pair ([3])
SHAPES = {"hs64-kv1": (64, 4, 4), "hs128-kv4": (128, 8, 2), "hs96-kv1": (96, 4, 4), "hs64-kv8": (64, 16, 2)}
ONE_LAUNCH = ("hs64-kv1", "hs128-kv4")
TREES = {
    "chain5": [-1, 0, 1, 2, 3],
    "star7": [-1] + [0] * 7,
    "bin15": [-1] + [(i - 1) // 2 for i in range(1, 15)],                # crosses an 8-row tile
    "tree64": [-1] + [(i - 1) // 3 for i in range(1, 64)],
}
# which child of node a (of nk children) carries a's greedy id: full path accepted / the accepted child is never the first sibling / rejected at the root
POLICY = {"first": lambda a, nk: 0, "last": lambda a, nk: nk - 1, "none": lambda a, nk: None if a == 0 else 0}


@pytest.fixture(scope="module")
def planmod():
    from importlib import import_module
    ge.load_package()
    return import_module(ge.PKG_NAME + ".plan"), import_module(ge.PKG_NAME + ".hip")


_MODELS = {}


def model(pkg, shape, ctx=CTX):
    if (shape, ctx) not in _MODELS:
        hs, heads, kv = SHAPES[shape]
        cfg = pkg.synth.ModelConfig(**{**pkg.synth.CONFIGS["tiny-llama"].__dict__, "head_size": hs, "n_heads": heads, "n_kv_heads": kv, "ctx": ctx})
        m = pkg.synth.make_numpy(cfg, seed=61)
        _MODELS[(shape, ctx)] = (m, pkg.javarand.bench_tokens(cfg.vocab, ctx))
    return _MODELS[(shape, ctx)]


def along(o, orc, p0, toks):
    """the oracle forwarded linearly on toks at p0, p0 + 1, ... -> the greedy id of the last row"""
    for j, t in enumerate(toks):
        lg = o.forward(t, p0 + j)
    return orc.argmax(lg)


def draft_tree(o, orc, V, p0, root, parents, policy):
    """tokens of the tree and what the rule gives for them: (tokens, positions, accepted path, token)"""
    n = len(parents)
    kids = {a: [i for i in range(n) if parents[i] == a] for a in range(n)}
    tokens, greedy, paths = [root] + [None] * (n - 1), [None] * n, [[0]] + [None] * (n - 1)
    for a in range(n):                                   # a parent precedes its children: tokens[a] and paths[a] are set
        greedy[a] = along(o, orc, p0, [tokens[j] for j in paths[a]])
        hit = POLICY[policy](a, len(kids[a]))
        for k, c in enumerate(kids[a]):
            tokens[c] = greedy[a] if k == hit else (greedy[a] + 1 + k) % V
            paths[c] = paths[a] + [c]
    a = 0
    while [c for c in kids[a] if tokens[c] == greedy[a]]:
        a = [c for c in kids[a] if tokens[c] == greedy[a]][0]
    along(o, orc, p0, [tokens[j] for j in paths[a]])     # leaves the oracle's K / V rows of the accepted path behind
    return tokens, [p0 + len(paths[i]) - 1 for i in range(n)], paths[a], greedy[a]


def run_case(pkg, orc, planmod, shape, trees, ctx=CTX):
    """trees: [(tree name, policy, p0)], tree r on sequence r"""
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
    rows = list(plan.attn_rows())
    assert rows == ([0, len(toks), 0, 0] if shape in ONE_LAUNCH and ctx == CTX else [0, 0, 0, len(toks)]), rows
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
    return res, want


CASES = [(shape, tree, policy, p0) for shape in ONE_LAUNCH
         for tree, policy in (("chain5", "first"), ("star7", "last"), ("bin15", "last"), ("tree64", "first")) for p0 in (0, 5, 70)]
CASES += [(shape, "star7", "none", 5) for shape in ONE_LAUNCH]
CASES += [(shape, tree, policy, p0) for shape in ("hs96-kv1", "hs64-kv8") for tree, policy in (("bin15", "last"), ("star7", "none")) for p0 in (5, 70)]
CASES += [(shape, tree, "first", p0) for shape in ("hs96-kv1", "hs64-kv8") for tree, p0 in (("chain5", 0), ("tree64", 0), ("tree64", 70))]


@pytest.mark.parametrize("shape,tree,policy,p0", CASES)
def test_one_tree(pkg, orc, planmod, shape, tree, policy, p0):
    res, want = run_case(pkg, orc, planmod, shape, [(tree, policy, p0)])
    acc = len(want[0][3]) - 1
    depth = {"chain5": 4, "star7": 1, "bin15": 3, "tree64": 4}[tree]      # the path of first / last children ends at a leaf of that depth
    assert acc == (0 if policy == "none" else depth)
    if policy == "last" and tree != "chain5":
        assert want[0][3][1] != want[0][0] + 1                         # the accepted child is not the first sibling: its rows were moved


@pytest.mark.parametrize("shape", ONE_LAUNCH + ("hs64-kv8",))
def test_two_trees_of_two_sequences_at_different_depths(pkg, orc, planmod, shape):
    run_case(pkg, orc, planmod, shape, [("bin15", "last", 70), ("star7", "first", 3)])


def test_a_chain_is_a_run_of_forward_batch_verify(pkg, orc, planmod):
    plan_mod, _ = planmod
    m, prompt = model(pkg, "hs64-kv1")
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size=16, n_seqs=2)
    o = orc.COracle(m)
    o.prefill(prompt[:5], 0)
    for s in (0, 1):
        plan.prefill_seq(s, prompt[:5], 0)
    toks, poss, _, _ = draft_tree(o, orc, m.cfg.vocab, 5, prompt[5], TREES["chain5"], "first")
    toks[3] = (toks[3] + 1) % m.cfg.vocab                               # the third draft is wrong: two stand
    res, path = plan.forward_batch_verify_tree(toks, [0] * 5, poss, TREES["chain5"])
    lin = plan.forward_batch_verify(toks, [1] * 5, poss)
    assert (int(res["accepted"][0]), int(res["token"][0])) == (int(lin["accepted"][0]), int(lin["token"][0])) and int(res["accepted"][0]) == 2
    assert path.tolist() == [0, 1, 2, -1, -1]
    for l in range(m.cfg.n_layers):
        for p in range(5, 10):                                          # every row of the run, the dead ones included: same slots, same values
            assert all(np.array_equal(a, b) for a, b in zip(plan.kv_seq(0, l, p), plan.kv_seq(1, l, p))), (l, p)
    plan.freeTornadoExecutionPlan()


def test_a_deep_prefix_runs_the_masked_windows(pkg, orc, planmod, monkeypatch):
    """p0 = 1030 is past the depth (511 at head size 128, kvMul 4) to which a tree's score rows fit LDS, so the step takes the masked per-row
    pair; GL3_ATTN_WINDOW=1024 (read in gl3_create) puts its rows (1031 .. 1045 scores) past the LDS window of the masked softmax: the
    sequential sum is carried across two windows and the tree's slots lie in the second."""
    monkeypatch.setenv("GL3_ATTN_WINDOW", "1024")
    run_case(pkg, orc, planmod, "hs128-kv4", [("bin15", "last", 1030)], ctx=1100)


BAD = {      # on tokens [3, 4, 5, 6, 7], one sequence, chain positions 5 .. 9 unless said otherwise
    "n > max_batch": dict(n=9), "token out of range": dict(tokens=[3, 4, 512, 6, 7]), "sequence out of range": dict(seqs=[2] * 5),
    "null parents": dict(parents=None), "first row with a parent": dict(parents=[0, 0, 1, 2, 3]), "later row without one": dict(parents=[-1, 0, -1, 2, 3]),
    "parent not earlier": dict(parents=[-1, 0, 2, 2, 3]), "parent in another tree": dict(seqs=[0, 0, 0, 1, 1], parents=[-1, 0, 1, -1, 2], poss=[5, 6, 7, 0, 8]),
    "position not the parent's + 1": dict(poss=[5, 6, 7, 7, 9]), "duplicate siblings": dict(tokens=[3, 4, 4, 6, 7], parents=[-1, 0, 0, 1, 2], poss=[5, 6, 6, 7, 7]),
    "p0 + rows > ctx": dict(poss=[CTX - 4 + i for i in range(5)]), "a sequence twice": dict(seqs=[0, 0, 1, 0, 0], parents=[-1, 0, -1, -1, 3], poss=[5, 6, 0, 5, 6]),
    "65 rows": dict(tokens=list(range(65)), seqs=[0] * 65, parents=[-1] + [0] * 64, poss=[5] + [6] * 64),
}


@pytest.mark.parametrize("what", sorted(BAD) + ["max_batch 1"])
def test_refusals(pkg, planmod, what):
    plan_mod, hip = planmod
    m, prompt = model(pkg, "hs64-kv1")
    plan = plan_mod.HipMasterPlan(m, prefill_batch_size={"n > max_batch": 8, "max_batch 1": 1}.get(what, 80), n_seqs=2)
    plan.prefill_seq(0, prompt[:6], 0)
    before = np.concatenate(plan.kv_seq(0, 1, 5))
    bad = BAD.get(what, {})
    n = bad.get("n", 5)
    args = [bad.get("tokens", list(range(3, 3 + n))), bad.get("seqs", [0] * n), bad.get("poss", list(range(5, 5 + n))), bad.get("parents", list(range(-1, n - 1)))]
    if args[3] is None:
        arr = [np.ascontiguousarray(a, np.int32) for a in args[:3]]
        res, path, cnt = np.zeros(n, plan_mod.VERIFY_DTYPE), np.zeros(n, np.int32), np.zeros(1, np.int32)
        code = hip.lib().gl3_forward_batch_verify_tree(plan._ctx, *[a.ctypes.data for a in arr], None, n, res.ctypes.data, path.ctypes.data,
                                                       cnt.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    else:
        with pytest.raises(hip.Gl3Error) as ei:
            plan.forward_batch_verify_tree(*args)
        code = ei.value.code
    assert code == (hip.E_UNSUPPORTED if what == "max_batch 1" else hip.E_ARG), what
    assert np.array_equal(before, np.concatenate(plan.kv_seq(0, 1, 5)))      # nothing was staged or enqueued: the row is untouched
    plan.freeTornadoExecutionPlan()
