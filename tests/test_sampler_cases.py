"""tests/sampler_cases.py on the oracle alone (no GPU): every case of the table hits the boundary its tag names.

For each case the probabilities are the C oracle's (orc.sample(.., want_probs=True)), held equal to the NumPy ones the case was aimed with,
and every entry of the case's aim is asserted on them: n0, the truncation rank, exceeded / not exceeded, the sampled rank, fell through or
not, tied or not, in the heap's own tail or not, subnormal and zero counts, the chunk a categorical pick lands in.  For every top-p case
that is neither tied nor in the heap's tail the index the sorted restatement puts at the sampled rank must be orc.sample's id (the heap's),
for every categorical case the cdf walk's; test_the_heap_sorts_all_but_its_last_three holds the rule itself against the heap.  The coverage tests
then assert that the table as a whole crosses every boundary it was written for, so tests/test_gpu_sampler_edges.py cannot pass on cases
that miss theirs."""
import numpy as np
import pytest

import sampler_cases as sc

F32 = np.float32
TINY = np.finfo(F32).tiny


@pytest.fixture(scope="module")
def judged(orc):
    """{V: [(case, oracle probabilities, oracle id, Sorted or Picked)]}, computed once"""
    out = {}
    for V in sc.VOCABS:
        rows = []
        for c in sc.cases(V):
            tok, probs = orc.sample(c.logits, c.temperature, c.topp, c.coin, want_probs=True)
            got = sc.sorted_topp(probs, c.topp, c.coin) if sc.is_topp(c.temperature, c.topp) else sc.categorical(probs, c.coin)
            rows.append((c, probs, tok, got))
        out[V] = rows
    return out


@pytest.mark.parametrize("V", sc.VOCABS)
def test_every_case_hits_its_aim(judged, V):
    tags = set()
    for c, probs, tok, got in judged[V]:
        assert c.tag not in tags, c.tag
        tags.add(c.tag)
        assert c.V == V and c.logits.dtype == F32 and np.all(np.isfinite(c.logits)) and 0 <= c.coin < 1 and c.temperature > 0
        assert np.array_equal(probs, sc.probs_of(c.logits, c.temperature)), c.tag
        for key, want in c.aim.items():
            if key == "subnormal":
                assert np.count_nonzero((probs > 0) & (probs < TINY)) == want, (c.tag, key)
            elif key == "zero":
                assert np.count_nonzero(probs == 0) == want, (c.tag, key)
            elif key == "cutoff_index":
                order, _ = sc.sorted_candidates(probs, c.topp)
                assert probs[want] == sc.cutoff_of(c.topp, V) and order[-1] == want and np.count_nonzero(probs == probs[want]) == 1, c.tag
            else:
                assert getattr(got, key) == want, (c.tag, key, getattr(got, key), want)
        if isinstance(got, sc.Picked) or not got.host:
            assert got.index == tok, (c.tag, got, tok)


def topp_rows(judged, V=None):
    return [(c, g) for v in ([V] if V else sc.VOCABS) for c, _, _, g in judged[v] if isinstance(g, sc.Sorted)]


def test_the_heap_sorts_all_but_its_last_three(orc):
    """The rule sorted_prefix states, against the reference's heap on 4000 random rows of 1 .. 13 distinct candidates: while the sum exceeds
    topp within the sorted prefix the stable sort names the heap's token, every time; past it the two disagree on some rows (so the
    prefix is no shorter than it has to be by much: the heap's tail is real)."""
    rng = np.random.default_rng(0)
    device = tail = differ = 0
    for _ in range(4000):
        V = 16 * int(rng.integers(1, 4))
        K = int(rng.integers(1, 14))
        lg = np.full(V, sc.LOW, F32)
        lg[rng.permutation(V)[:K]] = rng.standard_normal(K).astype(F32)
        topp, coin = float(rng.choice([0.3, 0.6, 0.9, 0.99, 0.9999])), float(F32(rng.random() * 0.999))
        tok, p = orc.sample(lg, 1.0, topp, coin, want_probs=True)
        g = sc.sorted_topp(p, topp, coin)
        if not g.host:
            device += 1
            assert g.index == tok, (lg.tolist(), topp, coin, g, tok)
        elif not g.tied:
            tail += 1
            differ += g.index != tok
    assert device > 1000 and tail > 1000 and differ > 0
    assert [sc.sorted_prefix(n) for n in (1, 2, 3, 4, 5, 9)] == [1, 2, 1, 1, 2, 6]


def test_candidate_counts(judged):
    """every K < V of the table comes out as n0 exactly — the chunk phase 0 sums is min(4096, n0) ranks long, so the naive / exact split and
    the trailing 0, 1 or 3 elements are those of n0 itself — in draws the device answers and, from K = 3, in draws it must hand to the host
    because the sum reaches the heap's tail; the last truncation point the device answers (n0 - 4) with the coin on it"""
    for V in sc.VOCABS:
        rows = topp_rows(judged, V)
        assert {g.n0 for c, g in rows if not g.host} >= {K for K in sc.COUNTS if K < V}, V
        assert {g.n0 for c, g in rows if g.heap_tail and not g.tied} >= {K for K in sc.COUNTS if 3 <= K < V}, V
        assert {g.n0 for c, g in rows if not g.host and g.last == g.rank == g.n0 - 4} >= {K for K in sc.COUNTS if 5 <= K < V}, V
        assert {g.n0 for c, g in rows if g.heap_tail and g.last == g.n0 - 3} >= {K for K in sc.COUNTS if 5 <= K < V}, V
        assert 1 in {g.n0 for c, g in rows}
    n0s = {g.n0 for c, g in topp_rows(judged)}
    assert {k for k in n0s if k % 4} and {k for k in n0s if k < sc.EXACT_FROM} and {k for k in n0s if k > sc.CHUNK}


def test_truncation_ranks(judged):
    for V in (4112, 9232):
        rows = topp_rows(judged, V)
        lasts = {g.last for c, g in rows if g.exceeded and not g.host}
        assert {0, sc.CHUNK - 1, sc.CHUNK} <= lasts, V
        # phase 1 ends inside a chunk, at the end of one, and one rank into the next
        assert {(g.last + 1) % sc.CHUNK for c, g in rows} >= {0, 1}
        # the coin on both sides of the chunk edge while the truncation is past it
        assert {g.rank for c, g in rows if g.last > sc.CHUNK and not g.host} >= {sc.CHUNK - 1, sc.CHUNK}
    for V in sc.VOCABS:
        rows = topp_rows(judged, V)
        assert any(g.exceeded and g.last == g.n0 - 1 and g.n0 > 1 for c, g in rows)
        assert any(g.rank == 0 and not g.host for c, g in rows) and any(g.rank == g.n0 - 1 and g.n0 > 1 for c, g in rows)
        # the top-p fall-through cannot be aimed at: coin <= 1 - 2^-24 and a normal cum make fl(coin * cum) < cum, the cdf at the truncation rank.
        # The largest coin (trunc-rank0) puts the product one f32 step under cum, as close as a draw gets
        assert not any(g.fell for c, g in rows), V
        assert any(c.coin == float(sc.BELOW_ONE) and sc.up(F32(F32(c.coin) * g.cum)) == g.cum and not g.host for c, g in rows), V


def test_never_exceeds(judged):
    """topp equal to the candidates' sum is not exceeded (every candidate kept); the f32 below it is, at the last rank"""
    for V in sc.VOCABS:
        never = {g.n0 for c, g in topp_rows(judged, V) if not g.exceeded}
        assert never >= {K for K in sc.COUNTS if 3 <= K < V}, (V, sorted(never))
        for c, g in topp_rows(judged, V):
            if not g.exceeded:
                assert g.last == g.n0 - 1 and g.cum == F32(c.topp) and 0 < c.topp < 1
            if c.tag.startswith("just-below-sum"):
                assert g.exceeded and g.last == g.n0 - 1 and sc.up(c.topp) == g.cum


def test_tie_borders(judged):
    for V in sc.VOCABS:
        rows = [(c, g) for c, g in topp_rows(judged, V) if c.tag.startswith("tie/")]
        kinds = {c.tag.split()[0][4:]: (c, g) for c, g in rows}
        assert set(kinds) == {"head", "head-last", "block-first", "block-last", "top-pair", "behind-top-pair"}
        for c, g in rows:
            p = sc.probs_of(c.logits, c.temperature)
            sv = p[sc.sorted_candidates(p, c.topp)[0]]
            assert np.count_nonzero(sv[:-1] == sv[1:]) > 0                           # the row has ties, whatever the sampled rank
        assert not any(g.heap_tail for c, g in rows)                                # host or device by the tie flag alone
        c, g = kinds["block-last"]
        sv = np.sort(sc.probs_of(c.logits, 1.0))[::-1]
        assert g.rank == g.last == g.n0 - 4 and g.tied and sv[g.rank - 1] == sv[g.rank] != sv[g.rank + 1]
        c, g = kinds["block-first"]
        sv = np.sort(sc.probs_of(c.logits, 1.0))[::-1]
        assert g.tied and sv[g.rank - 1] != sv[g.rank] == sv[g.rank + 1]
        c, g = kinds["top-pair"]
        assert g.rank == 0 and g.tied
        assert [kinds[k][1].tied for k in ("head", "head-last", "block-first", "behind-top-pair")] == [False, False, True, False]
    # a tied block across the chunk edge: its first rank is the last of chunk 0
    assert any(g.tied and g.rank == sc.CHUNK - 1 for c, g in topp_rows(judged, 4112))
    assert all(any("cutoff_index" in c.aim for c, g in topp_rows(judged, V)) for V in sc.VOCABS if V > 16)


def test_categorical_edges(judged):
    for V in sc.VOCABS:
        rows = [(c, p, g) for c, p, _, g in judged[V] if c.tag.startswith("cat/")]
        assert any(g.fell and g.index == V - 1 for c, p, g in rows) and any(g.index == 0 for c, p, g in rows)
        for c, p, g in rows:
            if g.fell:
                assert np.add.accumulate(p, dtype=F32)[-1] < 1 and p[V - 1] == 0
        for e in range(sc.CHUNK, V, sc.CHUNK):
            cdf = np.add.accumulate(rows[0][1], dtype=F32)
            at = {float(c.coin): g.index for c, p, g in rows}
            assert at[float(cdf[e - 1])] == e and at[float(sc.down(cdf[e - 1]))] == e - 1 and at[float(sc.up(cdf[e - 1]))] == e
    assert any(g.index >= sc.CHUNK for c, p, g in [(c, p, g) for c, p, _, g in judged[4112] if c.tag.startswith("cat/last-16")])


def test_value_rows(judged):
    """at V = 1008 the spread of 80 .. 104 below the maximum gives hundreds of f32-subnormal probabilities and a few zeros at T = 1,
    nothing but zeros at T = 0.02; maxima at index 0, V - 1, the first element of the last chunk, three times, +0 and -0"""
    for V in sc.VOCABS:
        rows = [(c, p) for c, p, _, g in judged[V] if c.tag.startswith("value/max-")]
        where = {int(np.argmax(c.logits)) for c, p in rows}
        assert {0, V - 1, ((V - 1) // sc.CHUNK) * sc.CHUNK} <= where
        assert any(np.count_nonzero(c.logits == c.logits.max()) == 3 and np.any(np.signbit(c.logits[c.logits == 0])) for c, p in rows)
        assert {c.temperature for c, p in rows} == {1.0, 0.02, 5.0}
        one = [(c, p) for c, p in rows if c.temperature == 1.0 and "subnormal" in c.aim]
        assert one and all(c.aim["subnormal"] > 0.5 * V and (c.aim["zero"] >= 1 or V == 16) for c, p in one)
        assert all(c.aim["zero"] == V - 1 for c, p in rows if c.temperature == 0.02 and "zero" in c.aim)
    c = next(c for c, p in [(c, p) for c, p, _, g in judged[1008] if c.tag.startswith("value/max-first T=1.0")])
    assert (c.aim["subnormal"], c.aim["zero"]) == (697, 2)


def test_sort_stability_rows(judged):
    for V in sc.VOCABS:
        rows = [(c, g) for c, g in topp_rows(judged, V) if c.tag.startswith("stability/")]
        assert [g.tied for c, g in rows] == [False, False, True] and [g.rank for c, g in rows] == [0, 0, 1]
        assert all(g.n0 == V and np.count_nonzero(c.logits == c.logits.max()) == 1 for c, g in rows)


def test_radix_tile_tails_and_scan_sizes():
    tiles = {V: -(-V // sc.RS_TILE) for V in sc.VOCABS}
    assert {V for V in sc.VOCABS if V % sc.RS_TILE == 16} == {16, 1040, 4112, 9232}    # a last tile with 16 valid elements
    assert min(tiles.values()) == 1 and max(tiles.values()) == 10                      # btp_scan over 256 .. 2560 entries
