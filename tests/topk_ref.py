"""NumPy restatement of the top-k / min-p / top-p sampler's contract (csrc/gl3_topk_sample.h, include/gpullama3_hip.h).  np.cumsum on
float32 is the strictly sequential f32 sum (tests/test_topk_sample_host.py holds it to a Python loop)."""
import numpy as np

F32 = np.float32


def sample(logits, top_k, temperature, topp, minp, coin):
    """-> (token, survivor ids [kk], their probabilities [kk], n_keep)"""
    l = np.asarray(logits, F32) + F32(0.0)
    T, topp, minp, coin = F32(temperature), F32(topp), F32(minp), F32(coin)
    kk = min(int(top_k), l.size)
    ids = np.argsort(-l, kind="stable")[:kk]
    v = (l[ids] / T).astype(F32)
    e = np.exp((v - v[0]).astype(np.float64)).astype(F32)
    p = (e / np.cumsum(e, dtype=F32)[-1]).astype(F32)
    m = kk
    if 0 < minp <= 1:
        cut = np.flatnonzero(~(p >= minp * p[0]))
        m = max(int(cut[0]), 1) if cut.size else kk
    c = np.cumsum(p[:m], dtype=F32)
    n_keep = m
    if 0 < topp < 1:
        over = np.flatnonzero(c > topp)
        n_keep = int(over[0]) + 1 if over.size else m
    hit = np.flatnonzero(coin * c[n_keep - 1] < c[:n_keep])
    return int(ids[hit[0] if hit.size else n_keep - 1]), ids.astype(np.int32), p, n_keep
