"""NumPy restatement of draft verification against a draft DISTRIBUTION (gl3_forward_batch_verify_dist / gl3_verify_rows_dist,
include/gpullama3_hip.h) and of the loop of tools/gl3_spec_draft_run.  The probabilities and the last row's sampler are verify_ref's; the
sequential sums of the residual are f32 np.cumsum, which accumulates left to right, as in verify_ref.resample."""
import numpy as np

import verify_ref as vr

F32 = np.float32


def accepts(p, q, d, coin):
    """accept iff coin * q[d] < p[d]: one f32 product, strictly less"""
    return bool(F32(coin) * F32(q[d]) < p[d])


def resample(p, q, coin, greedy_id):
    """The token a row emits after rejecting a draft drawn from q -> (token, which branch named it): r = max(p - q, 0), target = coin * S',
    'cdf' the first j with target < cdf_j, 'last' (no such j, S' > 0) the largest j with r[j] > 0, 'greedy' (S' == 0) the row's greedy id"""
    r = np.maximum(p - np.asarray(q, F32), F32(0.0)).astype(F32)
    cdf = np.cumsum(r, dtype=F32)
    if cdf[-1] == 0:
        return int(greedy_id), "greedy"
    hit = np.nonzero(F32(coin) * cdf[-1] < cdf)[0]
    if hit.size:
        return int(hit[0]), "cdf"
    return int(np.nonzero(r > 0)[0][-1]), "last"


def verify_run(logits, tokens, temperature, coins, q_rows, trace=None):
    """One run, as verify_ref.verify_run; q_rows[i]: the distribution (f32[vocab]) the draft of row i was drawn from, or None for a fixed
    token (verify_ref's one-hot rule).  trace: a list that receives the branch of a dist resample -> (accepted, token)"""
    m = len(tokens)
    if temperature == 0:
        return vr.verify_run(logits, tokens)
    for i in range(m):
        p = vr.probs(logits[i], temperature)
        if i + 1 == m:
            return i, vr.categorical(p, coins[i][1])
        d, q = int(tokens[i + 1]), q_rows[i]
        if q is None:
            if not F32(coins[i][0]) < p[d]:
                return i, vr.resample(p, d, coins[i][1])
        elif not accepts(p, q, d, coins[i][0]):
            tok, how = resample(p, q, coins[i][1], vr.first_max(logits[i]))
            if trace is not None:
                trace.append(how)
            return i, tok
    raise AssertionError("a run has at least one row")


def verify_rows(logits, tokens, run_rows, temperature, coins, q_slots, table):
    """Every run of a step -> [(accepted, token)]; q_slots: one entry per row (-1: a fixed token), table: {slot: f32[vocab]}.  The last row of
    a run and the rows of a greedy run never look at their entry"""
    out, r0 = [], 0
    for k, m in enumerate(run_rows):
        look = range(r0, r0 + m - 1) if temperature[k] > 0 else ()
        q_rows = [table[int(q_slots[i])] if i in look and q_slots[i] >= 0 else None for i in range(r0, r0 + m)]
        out.append(verify_run(logits[r0:r0 + m], tokens[r0:r0 + m], temperature[k], coins[r0:r0 + m], q_rows))
        r0 += m
    return out


def simulate_draft_run(prompt, target_forward, draft_forward, n_new, rng, draft=4, batch=16, temperature=0.0, draft_temperature=None, ctx=None):
    """The loop of tools/gl3_spec_draft_run.  target_forward / draft_forward(token, position) -> logits f32[vocab] of a model whose K / V rows
    below `position` are what earlier calls left (a CPU oracle each; both already hold the prompt but its last id); rng.next_float() the
    coin stream -> (generated, steps, drafted, accepted)"""
    T = temperature
    Td = T if draft_temperature is None else draft_temperature
    sampled = T > 0 and Td > 0
    ctx = len(prompt) + n_new if ctx is None else ctx
    gen, pos, last = [], len(prompt) - 1, prompt[-1]
    steps = drafted = accepted = 0
    while len(gen) < n_new and pos < ctx:
        k = min(draft, n_new - len(gen) - 1, ctx - 1 - pos, batch - 1)
        toks, q_rows = [last], []
        for j in range(k):
            lg = draft_forward(toks[j], pos + j)
            if sampled:
                q = vr.probs(lg, Td)
                toks.append(vr.categorical(q, rng.next_float()))
                q_rows.append(q)
            else:
                toks.append(vr.first_max(lg))
                q_rows.append(None)
        m = k + 1
        coins = [(rng.next_float(), rng.next_float()) for _ in range(m)] if T > 0 else [(0.0, 0.0)] * m
        rows = []

        class Lazy:                      # the rule stops at the first rejection: rows behind it are never forwarded through the oracle
            def __getitem__(self, i):
                while len(rows) <= i:
                    rows.append(target_forward(toks[len(rows)], pos + len(rows)))
                return rows[i]
        a, tok = verify_run(Lazy(), toks, T, coins, q_rows + [None])
        steps += 1; drafted += k; accepted += a
        gen += toks[1:a + 1] + [tok]
        if a == k and len(gen) < n_new and pos + k + 1 < ctx:
            draft_forward(toks[k], pos + k)          # the id at pos + k has not been through the draft model
        pos += a + 1
        last = tok
    return gen, steps, drafted, accepted
