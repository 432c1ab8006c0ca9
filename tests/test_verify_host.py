"""CPU-side checks of draft verification: the NumPy restatement of the rule (tests/verify_ref.py) against the oracle's samplers, and the
C-ABI surface (gl3_forward_batch_verify, gl3_verify_rows) — header, exports, ctypes mirror, HipMasterPlan, the native host's build rule."""
import ctypes
import os
import re

import numpy as np

import __graft_entry__ as ge
import verify_ref as vr

F32 = np.float32
NEW = ["gl3_forward_batch_verify", "gl3_verify_rows"]


def _hip():
    if not os.path.exists(os.path.join(ge.PKG_DIR, "libgpullama_hip.so")):
        ge.build()
    ge.load_package()
    from importlib import import_module
    return import_module(ge.PKG_NAME + ".hip")


def test_greedy_is_the_first_max_chain(orc):
    rng = np.random.default_rng(3)
    V, m = 48, 6
    lg = rng.standard_normal((m, V)).astype(F32)
    lg[2, 5] = lg[2, 30] = lg[2].max() + F32(1.0)                       # two equal maxima: the first one is the greedy id
    ids = [orc.argmax(r) for r in lg]
    assert ids[2] == 5 and ids == [vr.first_max(r) for r in lg]
    for wrong in range(m):                                              # the first wrong draft ends the chain; wrong == m - 1: every draft stands
        tokens = [7] + ids[:m - 1]
        if wrong < m - 1:
            tokens[wrong + 1] = (ids[wrong] + 1) % V
        assert vr.verify_run(lg, tokens) == (wrong, ids[wrong])
        assert vr.verify_rows(lg, tokens, [m]) == [(wrong, ids[wrong])]
    tokens = [7, ids[0], ids[1], 30, ids[3], ids[4]]                    # the draft sits on the second of the equal maxima: rejected
    assert vr.verify_run(lg, tokens) == (2, 5)
    assert vr.verify_run(lg[:1], [7]) == (0, ids[0])                    # a run of one row


def test_a_single_sampled_row_is_the_categorical_sampler(orc):
    rng = np.random.default_rng(4)
    V = 1008
    for T in (0.4, 1.0, 3.0):
        lg = (rng.standard_normal((1, V)) * 3).astype(F32)
        _, p = orc.sample(lg[0], T, 0.0, 0.5, want_probs=True)
        assert np.array_equal(vr.probs(lg[0], T), p)                    # the restatement draws from the oracle's probabilities
        for coin in (0.0, 0.25, 0.5, float(F32(1.0) - F32(2.0) ** -24)) + tuple(rng.random(20).astype(F32).tolist()):
            assert vr.verify_run(lg, [3], T, [(0.123, coin)]) == (0, orc.sample(lg[0], T, 0.0, coin)), (T, coin)


def test_the_emitted_token_is_never_the_rejected_draft(orc):
    rng = np.random.default_rng(5)
    V = 64
    coins = [0.0, 0.5, float(F32(1.0) - F32(2.0) ** -24)] + rng.random(200).astype(F32).tolist()
    for d in (0, V - 1, 17):
        lg = rng.standard_normal((2, V)).astype(F32)
        lg[0, d] = lg[0].max() + F32(2.0)                                # the draft is the likeliest token: a resample that ignored the
        p = vr.probs(lg[0], 1.0)                                        # exclusion would return it often
        for c in coins:
            a, tok = vr.verify_run(lg, [1, d], 1.0, [(float(p[d]), c), (0.0, 0.0)])      # accept coin == p[d]: rejected (strict <)
            assert a == 0 and tok != d and 0 <= tok < V, (d, c, tok)
        one = np.zeros(V, F32)
        one[d] = F32(1.0)                                                # S' == 0: no j with r < cdf_j, the largest index other than d
        assert vr.resample(one, d, 0.5) == (V - 2 if d == V - 1 else V - 1)
        below = float(np.nextafter(p[d], F32(0.0)))
        a, tok = vr.verify_run(lg, [1, d], 1.0, [(below, 0.3), (0.9, 0.3)])                # one ulp below p[d]: accepted
        assert (a, tok) == (1, vr.categorical(vr.probs(lg[1], 1.0), 0.3))


def test_the_lookup_drafts_what_followed_the_most_recent_match():
    h = [1, 2, 3, 9, 1, 2, 3, 4, 5, 6, 7, 1, 2, 3]
    assert vr.lookup_draft(h, 3, 4) == [4, 5, 6, 7]                      # the later occurrence of (1, 2, 3), not the one followed by 9
    assert vr.lookup_draft(h, 3, 2) == [4, 5]
    assert vr.lookup_draft(h, 3, 0) == []
    assert vr.lookup_draft([1, 2, 3, 4], 3, 4) == []                    # no earlier occurrence of any suffix
    assert vr.lookup_draft([5, 8, 5], 3, 4) == [8, 5]                    # falls back to g = 1; the proposal may run into the suffix itself
    assert vr.lookup_draft([5, 5], 3, 4) == [5]
    gen, steps, drafted, accepted = vr.simulate_spec_run([1, 2, 3, 1], [2, 3, 1, 7, 3, 1], 6, draft=2, ngram=2)
    assert gen == [2, 3, 1, 7, 3, 1] and (steps, drafted, accepted) == (4, 4, 2)


def test_the_header_declares_the_entries_and_the_record(pkg):
    hdr = open(os.path.join(ge.ROOT, "include", "gpullama3_hip.h")).read()
    assert re.search(r"typedef\s+struct\s*\{\s*int32_t\s+accepted\s*,\s*token\s*;\s*\}\s*gl3_verify_result\s*;", hdr)
    for name in NEW:
        assert re.search(r"GL3_API\s+int32_t\s+%s\s*\(" % name, hdr), name
    _hip()
    from importlib import import_module
    plan_mod = import_module(ge.PKG_NAME + ".plan")
    assert plan_mod.VERIFY_DTYPE.itemsize == 8 and plan_mod.VERIFY_DTYPE.names == ("accepted", "token")
    for name in ("forward_batch_verify", "verify_rows"):
        assert callable(getattr(plan_mod.HipMasterPlan, name))


def test_check_exports_lists_both_symbols(pkg):
    hip = _hip()
    names = hip.check_exports()                   # header == ctypes table == exported symbols
    raw = ctypes.CDLL(hip.SO_PATH)
    for name in NEW:
        assert name in names and name in hip._SIGS
        getattr(raw, name)
    L = hip.lib()
    assert L.gl3_forward_batch_verify(None, None, None, None, 1, None, None, None, None) == hip.E_ARG      # a null context, before any device
    assert L.gl3_verify_rows(None, None, None, None, 1, None, None, None) == hip.E_ARG


def test_the_makefile_builds_the_speculative_host(pkg):
    mk = open(os.path.join(ge.PKG_DIR, "csrc", "Makefile")).read()
    assert re.search(r"^all:.*\$\(SPEC_RUN\)", mk, re.M)
    assert re.search(r"^\$\(SPEC_RUN\):\s*\.\./\.\./tools/gl3_spec_run\.cpp\b", mk, re.M)
    assert os.path.exists(os.path.join(ge.ROOT, "tools", "gl3_spec_run.cpp"))
