"""CPU-side checks of draft verification against a draft distribution: properties of the NumPy restatement (tests/verify_dist_ref.py) that
follow from the rule itself, so none needs a tolerance; the crafted cases of the GPU test are what their names say; and the C-ABI surface
(header, exports, ctypes mirror, HipMasterPlan, the native host's build rule)."""
import ctypes
import os
import re

import numpy as np

import __graft_entry__ as ge
import verify_dist_cases as vc
import verify_dist_ref as vd
import verify_ref as vr

F32 = np.float32
TOP = vc.TOP
NEW = ["gl3_draft_probs_put", "gl3_draft_probs_put_host", "gl3_get_draft_probs", "gl3_forward_batch_verify_dist", "gl3_verify_rows_dist"]


def _hip():
    if not os.path.exists(os.path.join(ge.PKG_DIR, "libgpullama_hip.so")):
        ge.build()
    ge.load_package()
    from importlib import import_module
    return import_module(ge.PKG_NAME + ".hip")


def test_a_one_hot_q_is_the_one_hot_rule():
    rng = np.random.default_rng(11)
    V, T = 96, 0.8
    coins = [0.0, 0.5, TOP] + rng.random(40).astype(F32).tolist()
    for d in (0, V - 1, V - 2, 17):
        lg = rng.standard_normal((3, V)).astype(F32)
        p = vr.probs(lg[0], T)
        assert p[V - 1] > 0 and p[V - 2] > 0                             # both "no j" fallbacks name the same index
        one = np.zeros(V, F32)
        one[d] = F32(1.0)
        for accept in (0.0, float(p[d]), float(np.nextafter(p[d], F32(0))), TOP):
            for emit in coins:
                c = [(accept, emit), (0.3, emit), (0.9, emit)]
                tokens = [1, d, 5]
                assert vd.verify_run(lg, tokens, T, c, [one, None, None]) == vr.verify_run(lg, tokens, T, c), (d, accept, emit)


def test_the_emitted_token_is_never_the_rejected_draft():
    rng = np.random.default_rng(12)
    V, T = 64, 1.0
    coins = [0.0, 0.5, TOP] + rng.random(200).astype(F32).tolist()
    for d in (0, V - 1, 23):
        lg = rng.standard_normal((2, V)).astype(F32)
        lg[0, d] = lg[0].max() + F32(2.0)                                # the draft is the target's likeliest token and the draft model's
        q = vr.probs(rng.standard_normal(V).astype(F32), T)             # even likelier one: a resample that kept it would return it often
        q[d] = F32(1.0)
        for c in coins:
            trace = []
            a, tok = vd.verify_run(lg, [1, d], T, [(TOP, c), (0.0, 0.0)], [q, None], trace)
            assert a == 0 and tok != d and 0 <= tok < V and trace == ["cdf"], (d, c, tok, trace)


def test_q_equal_to_p_accepts_unless_p_of_the_draft_is_zero():
    rng = np.random.default_rng(13)
    V, T = 80, 0.9
    lg = rng.standard_normal((2, V)).astype(F32)
    lg[0, 30] = lg[0, 61] = lg[0].max() + F32(1.0)                       # two equal maxima: the first one is the greedy id
    lg[0, 7] = lg[0].min() - F32(300.0)
    p = vr.probs(lg[0], T)
    assert p[7] == 0 and vr.first_max(lg[0]) == 30
    for d in range(V):                                                  # min(1, p / q) = 1: the largest coin still accepts
        if d != 7:
            assert vd.accepts(p, p.copy(), d, TOP), d
    trace = []
    assert vd.verify_run(lg, [1, 7], T, [(TOP, TOP), (0.0, 0.0)], [p.copy(), None], trace) == (0, 30)      # S' == 0: the first maximum
    assert trace == ["greedy"]


def test_the_crafted_cases_are_what_their_names_say():
    for V in (1008, 4112, 9232):
        cases = vc.crafted(V, np.random.default_rng(V), 0.7)
        branches = {c[7] for c in cases}
        assert branches == {None, "cdf", "last", "greedy"}
        for case in cases:
            vc.check(case)


class _FakeModel:
    """logits that depend on everything a real model's would: the token, the position and the ids at the positions below"""
    def __init__(self, V, salt):
        self.V, self.salt, self.kv = V, salt, {}

    def __call__(self, token, pos):
        self.kv[pos] = token
        key = [self.salt] + [self.kv.get(i, -1) + 1 for i in range(pos + 1)]
        return (np.random.default_rng(key).standard_normal(self.V) * 2).astype(F32)


def test_the_simulated_host_loop_is_a_pure_function_of_its_inputs(pkg):
    V, prompt = 48, [3, 9, 4, 1]

    def run(T, Td, seed, draft=4):
        target, drafter = _FakeModel(V, 1), _FakeModel(V, 2)
        for i, t in enumerate(prompt[:-1]):
            target(t, i); drafter(t, i)
        return vd.simulate_draft_run(prompt, target, drafter, 24, pkg.javarand.L32X64MixRandom(seed), draft=draft, batch=8, temperature=T,
                                     draft_temperature=Td)
    for T, Td in ((0.8, None), (0.8, 0.0), (0.0, None), (1.2, 0.5)):
        a, b = run(T, Td, 7), run(T, Td, 7)
        assert a == b and len(a[0]) == 24 and a[2] >= a[3] and a[1] + a[3] == 24      # every step emits its accepted drafts and one more id
    assert run(0.8, None, 7)[0] != run(0.8, None, 8)[0]                  # the coins matter
    plain = run(0.0, None, 7, draft=0)
    assert plain[1:] == (24, 0, 0) and run(0.0, None, 7)[0] == plain[0]      # greedy: the target's own greedy ids, whatever is drafted


def test_the_header_declares_the_entries(pkg):
    hdr = open(os.path.join(ge.ROOT, "include", "gpullama3_hip.h")).read()
    for name in NEW:
        assert re.search(r"GL3_API\s+int32_t\s+%s\s*\(" % name, hdr), name
    assert "q(x) min(1, p(x) / q(x))" in hdr                            # the derivation stands beside the one-hot one
    _hip()
    from importlib import import_module
    plan_mod = import_module(ge.PKG_NAME + ".plan")
    for name in ("draft_probs_put", "draft_probs_put_host", "draft_probs", "forward_batch_verify_dist", "verify_rows_dist"):
        assert callable(getattr(plan_mod.HipMasterPlan, name))


def test_check_exports_lists_the_symbols(pkg):
    hip = _hip()
    names = hip.check_exports()                   # header == ctypes table == exported symbols
    raw = ctypes.CDLL(hip.SO_PATH)
    for name in NEW:
        assert name in names and name in hip._SIGS
        getattr(raw, name)
    L = hip.lib()
    assert L.gl3_draft_probs_put(None, 0, None) == hip.E_ARG            # a null context, before any device
    assert L.gl3_draft_probs_put_host(None, 0, None) == hip.E_ARG
    assert L.gl3_get_draft_probs(None, 0, None) == hip.E_ARG
    assert L.gl3_forward_batch_verify_dist(None, None, None, None, 1, None, None, None, None, None) == hip.E_ARG
    assert L.gl3_verify_rows_dist(None, None, None, None, 1, None, None, None, None) == hip.E_ARG


def test_the_makefile_builds_the_draft_model_host(pkg):
    mk = open(os.path.join(ge.PKG_DIR, "csrc", "Makefile")).read()
    assert re.search(r"^all:.*\$\(SPEC_DRAFT_RUN\)", mk, re.M)
    assert re.search(r"^\$\(SPEC_DRAFT_RUN\):\s*\.\./\.\./tools/gl3_spec_draft_run\.cpp\b", mk, re.M)
    src = open(os.path.join(ge.ROOT, "tools", "gl3_spec_draft_run.cpp")).read()
    assert re.findall(r'#include\s+"([^"]+)"', src) == ["../include/gpullama3_hip.h"]      # the public header and the standard library only
