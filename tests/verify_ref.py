"""NumPy restatement of the draft-verification rule of gl3_forward_batch_verify / gl3_verify_rows (include/gpullama3_hip.h), and of the
prompt-lookup drafting of tools/gl3_spec_run.  The probabilities are oracle_np.softmax (FloatTensor.softmaxInPlace: max, exp in double, the
strictly sequential f32 sum, divide); the sequential sums of the resample are f32 np.cumsum, which accumulates left to right."""
import numpy as np

from oracle import oracle_np

F32 = np.float32


def probs(row, temperature):
    """softmaxInPlace(row / T)"""
    return oracle_np.softmax((np.asarray(row, F32) / F32(temperature)).astype(F32))


def first_max(row):
    """Sampler.TENSOR_ARGMAX: the first index of the maximum"""
    return int(np.argmax(np.asarray(row, F32)))


def categorical(p, coin):
    """CategoricalSampler.sampleToken: the first index whose f32 cdf exceeds the coin, else the last index"""
    hit = np.nonzero(F32(coin) < np.cumsum(p, dtype=F32))[0]
    return int(hit[0]) if hit.size else p.size - 1


def resample(p, d, coin):
    """The token a row emits after rejecting draft d: q = p with q[d] = 0f, r = coin * S', the first j with r < cdf_j, else the largest
    index other than d"""
    q = p.copy()
    q[d] = F32(0.0)
    cdf = np.cumsum(q, dtype=F32)
    r = F32(coin) * cdf[-1]
    hit = np.nonzero(r < cdf)[0]
    return int(hit[0]) if hit.size else (p.size - 2 if d == p.size - 1 else p.size - 1)


def verify_run(logits, tokens, temperature=0.0, coins=None):
    """One run: logits [m][vocab], tokens [m] = the last real token and m - 1 drafts, coins [m][2] = (accept, emit) per row
    -> (accepted, token)"""
    m = len(tokens)
    for i in range(m):
        d = int(tokens[i + 1]) if i + 1 < m else None
        if temperature == 0:
            g = first_max(logits[i])
            if d is None or g != d:
                return i, g
            continue
        p = probs(logits[i], temperature)
        if d is None:
            return i, categorical(p, coins[i][1])
        if not F32(coins[i][0]) < p[d]:
            return i, resample(p, d, coins[i][1])
    raise AssertionError("a run has at least one row")


def verify_rows(logits, tokens, run_rows, temperature=None, coins=None):
    """Every run of a step -> [(accepted, token)]; temperature: one per run, None = greedy everywhere"""
    out, r0 = [], 0
    for k, m in enumerate(run_rows):
        t = 0.0 if temperature is None else temperature[k]
        out.append(verify_run(logits[r0:r0 + m], tokens[r0:r0 + m], t, None if coins is None else coins[r0:r0 + m]))
        r0 += m
    return out


def lookup_draft(history, ngram, k):
    """tools/gl3_spec_run: for g = ngram down to 1, the most recent earlier occurrence of the last g ids; the up-to-k ids behind it"""
    n = len(history)
    if k <= 0:
        return []
    for g in range(min(ngram, n - 1), 0, -1):
        tail = history[n - g:]
        for s in range(n - g - 1, -1, -1):
            if history[s:s + g] == tail:
                return history[s + g:s + g + k]
    return []


def simulate_spec_run(prompt, greedy_ids, n_new, draft=4, ngram=3, batch=16, ctx=None, stop=()):
    """The loop of tools/gl3_spec_run over a KNOWN greedy continuation (greedy_ids: at least n_new ids of plain greedy decoding behind the
    prompt): a pure function of ids -> (generated, steps, drafted, accepted)"""
    history, gen = list(prompt), []
    ctx = len(prompt) + n_new if ctx is None else ctx
    pos, steps, drafted, accepted, stopped = len(prompt) - 1, 0, 0, 0, False
    while not stopped and len(gen) < n_new and pos < ctx:
        k = min(draft, n_new - len(gen) - 1, ctx - 1 - pos, batch - 1)
        dr = lookup_draft(history, ngram, k)
        a = 0
        while a < len(dr) and dr[a] == greedy_ids[len(gen) + a]:
            a += 1
        steps += 1; drafted += len(dr); accepted += a
        for tok in dr[:a] + [greedy_ids[len(gen) + a]]:
            gen.append(tok); history.append(tok)
            if tok in stop:
                stopped = True
                break
        pos += a + 1
    return gen, steps, drafted, accepted
