"""Crafted runs for gl3_verify_rows_dist (tests/test_gpu_verify_dist.py runs them on the GPU, tests/test_verify_dist_host.py checks on the CPU
that each is what its name says): logits and draft distributions at the edges of the rule, for a vocabulary V of one, two or three
4096-element chunks."""
import numpy as np

import verify_dist_ref as vd
import verify_ref as vr

F32 = np.float32
TOP = float(F32(1.0) - F32(2.0) ** -24)                   # the largest coin rng.nextFloat(1f) can give


def crafted(V, rng, T):
    """[(what, logits [m][V], tokens [m], temperature, coins [m][2], q_rows [m] (f32[V] or None = a fixed token), the `accepted` the case is
    built to give, the branch a dist resample must take or None)]"""
    cases = []

    def rows(m):
        return (rng.standard_normal((m, V)) * 3).astype(F32)

    def softq(m):
        return [vr.probs(r, T) for r in rows(m)]

    def add(what, lg, tokens, coins, q_rows, accepted, branch=None, temp=T):
        q_rows = list(q_rows) + [None] * (len(tokens) - len(q_rows))
        cases.append((what, lg.copy(), [int(t) for t in tokens], temp, np.asarray(coins, F32).reshape(len(tokens), 2), q_rows, accepted, branch))

    # q = the softmax of a second random row.  Accept coin 0 accepts wherever p[d] > 0; the largest coin rejects a draft with q[d] > p[d]
    lg, q = rows(4), softq(3)
    p = [vr.probs(r, T) for r in lg]
    likely = [int(np.argmax(p[i] - q[i])) for i in range(3)]           # p > q: accepted by every coin
    unlikely = [int(np.argmax(q[i] / np.maximum(p[i], F32(1e-30)))) for i in range(3)]      # q >> p: rejected by a coin near 1
    add("all accepted", lg, [3] + likely, [(TOP, .9), (TOP, .9), (TOP, .9), (.9, .37)], q, 3)
    add("rejection at row 0", lg, [3, unlikely[0], likely[1], likely[2]], [(TOP, .61), (0, .9), (0, .9), (.9, .37)], q, 0, "cdf")
    add("rejection mid-run", lg, [3, likely[0], unlikely[1], likely[2]], [(TOP, .9), (TOP, .23), (0, .9), (.9, .37)], q, 1, "cdf")
    # the accept boundary: q[d] = 0.5 makes coin * q[d] an exact halving, so the coin 2 p[d] gives equality (reject), one ulp below accepts
    lg, q = rows(2), softq(1)
    d = V - 3
    pd = vr.probs(lg[0], T)[d]
    assert 0 < pd < 0.25
    q[0][d] = F32(0.5)
    add("accept coin * q[d] == p[d]", lg, [5, d], [(float(F32(2.0) * pd), .5), (.9, .37)], q, 0, "cdf")
    add("accept coin * q[d] one ulp below p[d]", lg, [5, d], [(float(np.nextafter(F32(2.0) * pd, F32(0))), .5), (.9, .37)], q, 1)
    # q[d] == 0: accepted iff p[d] > 0, by every coin
    lg, q = rows(2), softq(1)
    q[0][11] = F32(0.0)
    assert vr.probs(lg[0], T)[11] > 0
    add("q[d] == 0 with p[d] > 0", lg, [5, 11], [(TOP, .5), (.9, .37)], q, 1)
    lg[0, 11] = lg[0].min() - F32(200.0)
    assert vr.probs(lg[0], T)[11] == 0
    add("q[d] == 0 with p[d] underflowed to 0", lg, [5, 11], [(0.0, .5), (.9, .37)], q, 0, "cdf")
    # q bitwise equal to p.  coin < 1 makes coin * p[d] < p[d] for every normal p[d] > 0 (min(1, p / q) = 1: always accepted), so the
    # rejection needs p[d] == 0; then r == 0 everywhere, S' == 0 and the row's greedy id (the first of two equal maxima) is emitted
    lg = rows(2)
    lg[0, 40] = lg[0, V - 9] = lg[0].max() + F32(1.0)
    lg[0, 9] = lg[0].min() - F32(200.0)
    p0 = vr.probs(lg[0], T)
    assert p0[9] == 0 and p0[V - 5] > 2.0 ** -100
    add("q == p, a draft with p[d] > 0 and the largest coin", lg, [5, V - 5], [(TOP, .5), (.9, .37)], [p0.copy()], 1)
    add("q == p, S' == 0: the greedy id", lg, [5, 9], [(TOP, .5), (.9, .37)], [p0.copy()], 0, "greedy")
    # no j with target < cdf_j while S' > 0: coin * S' == S' needs a subnormal S' (a normal S' times a coin < 1 rounds below S').  q == p
    # except at j0 in the FIRST chunk, where q is one ulp below a p of about 2^-108: r[j0] = 2^-131, everything else 0.  The draft sits in the
    # last chunk with q[d] = 2 p[d], rejected by the largest coin
    lg = rows(2)
    j0, d = 77, V - 2
    lg[0, j0] = lg[0].max() - F32(75.0 * T)
    p0 = vr.probs(lg[0], T)
    q0 = p0.copy()
    q0[j0] = np.nextafter(p0[j0], F32(0))
    q0[d] = F32(2.0) * p0[d]
    assert 0 < p0[j0] - q0[j0] < 2.0 ** -126 and p0[d] > 0
    add("emit coin TOP, the residual's last positive entry in the first chunk", lg, [5, d], [(TOP, TOP), (.9, .37)], [q0], 0, "last")
    # the draft in the first chunk, the hit in the last one: q takes the residual away everywhere but behind the last chunk's start
    lg = rows(2)
    p0 = vr.probs(lg[0], T)
    q0 = p0.copy()
    lo = (V - 1) // 4096 * 4096
    q0[lo + 5:] = F32(0.0)
    q0[3] = F32(1.0)
    add("d in the first chunk, the hit in the last", lg, [5, 3], [(TOP, .5), (.9, .37)], [q0], 0, "cdf")
    # one-hot q: the one-hot rule (compared against plan.verify_rows too); the last two probabilities are > 0, so both fallbacks agree
    lg = rows(3)
    for d, emit in ((0, 0.0), (V - 1, TOP), (17, 0.5)):
        one = np.zeros(V, F32)
        one[d] = F32(1.0)
        pd = float(vr.probs(lg[0], T)[d])
        add("one-hot q, d = %d, rejected, emit coin %r" % (d, emit), lg, [5, d, 8], [(pd, emit), (.9, .37), (.1, .2)], [one, None], 0, "cdf")
        add("one-hot q, d = %d, accepted" % d, lg[:2], [5, d], [(float(np.nextafter(F32(pd), F32(0))), emit), (.9, emit)], [one], 1)
    # greedy runs and fixed-token rows inside sampled runs never look at a distribution
    lg = rows(3)
    best = [int(np.argmax(r)) for r in lg]
    add("greedy run", lg, [3, best[0], best[1]], np.zeros((3, 2)), [], 2, temp=0.0)
    q = softq(1)
    add("a fixed-token row, then a row with q", lg, [3, best[0], best[1]], [(0, .9), (0, .4), (.9, .37)], [None, q[0]], 2)
    add("a run of one row", lg[:1], [7], [(.5, .31)], [], 0)
    return cases


def check(case):
    """the restatement's answer for a case, after asserting that the case is what its name says -> (accepted, token)"""
    what, lg, tokens, temp, coins, q_rows, accepted, branch = case
    trace = []
    want = vd.verify_run(lg, tokens, temp, coins, q_rows, trace)
    assert want[0] == accepted, (what, want)
    assert trace == ([branch] if branch else []), (what, trace)
    if branch:
        assert want[1] != tokens[want[0] + 1] or branch == "greedy", what      # the rejected draft does not come back
    return want
